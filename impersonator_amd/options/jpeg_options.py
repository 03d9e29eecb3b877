"""Command-line flags of the device JPEG writer (csrc/jpeg.hip, util.jpeg_bytes), for the drivers that write frames:
run_imitator.py, run_animate.py and run_mesh.py.  Every flag of TestOptions stays as it is; these default to off."""
from .test_options import TestOptions


def add_jpeg_arguments(parser):
    parser.add_argument('--device_jpeg', action='store_true', default=False,
                        help='encode the written frames as JPEG on the device (only the finished streams come to the host)')
    parser.add_argument('--jpeg_quality', type=int, default=75, help='--device_jpeg: quality 1..100')
    parser.add_argument('--jpeg_subsampling', type=int, default=420, choices=[420, 444], help='--device_jpeg: 4:2:0 or 4:4:4')


class JpegOptions(TestOptions):
    """TestOptions + --device_jpeg, --jpeg_quality, --jpeg_subsampling and, for run_imitator.py, --save_video / --fps"""

    def initialize(self):
        super().initialize()
        add_jpeg_arguments(self._parser)
        self._parser.add_argument('--save_video', type=str, default='',
                                  help='with --device_jpeg: also write the sequence as one Motion-JPEG .avi file')
        self._parser.add_argument('--fps', type=float, default=25.0, help='--save_video: frames per second')
