"""Command-line flags of motion-driven appearance transfer (run_animate.py): every flag of TestOptions, unchanged, plus the
reference subject whose parts are put on the source."""
from .test_options import TestOptions


class AnimateOptions(TestOptions):
    def initialize(self):
        super().initialize()
        p = self._parser
        p.add_argument('--ref_path', type=str, default='',
                       help='image of the reference subject: the parts named by --swap_part come from it (the person who moves, '
                            'the background and the other parts are those of --src_path)')
