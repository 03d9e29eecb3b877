"""Command-line flags of evaluate.py (the paired metrics of the reference's evaluate.py: SSIM, PSNR, SSPE).  Every flag of
TestOptions stays as it is; `--hmr_model`, when it names a checkpoint of the HMR regressor, adds SSPE."""
from .test_options import TestOptions


class EvalOptions(TestOptions):
    def initialize(self):
        super().initialize()
        p = self._parser
        p.add_argument('--against', type=str, default='', choices=['', 'fp32', 'target'],
                       help="ground truth: 'fp32' = the same sequence through the exact-fp32 generator (default under --synthetic "
                            "without --tgt_path), 'target' = the frames of --tgt_path (self-imitation)")
        p.add_argument('--quantize', action='store_true', default=False,
                       help='score what an 8-bit writer would have stored (truncating uint8 round trip; JPEG loss is not modelled)')
