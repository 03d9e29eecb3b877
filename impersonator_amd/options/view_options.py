"""Command-line flags of novel view synthesis (run_view.py): every flag of TestOptions, unchanged, plus the view flags the
reference keeps in options/test_options.py:37-40."""
from .test_options import TestOptions


class ViewOptions(TestOptions):
    def initialize(self):
        super().initialize()
        p = self._parser
        p.add_argument('--view_params', type=str, default='R=0,90,0/t=0,0,0',
                       help='R=<degrees x,y,z>/t=<x,y,z>; the turntable schedule overrides R and keeps t')
        p.add_argument('--T_pose', action='store_true', default=False,
                       help='view in T pose or not (the reference defines this flag and never reads it; neither does this code)')
        p.add_argument('--num_views', type=int, default=16, help='views of the turntable (extension; the reference has 16)')
