"""Command-line flags of evaluate.py (the metrics of the reference's evaluate.py: SSIM, PSNR, SSPE, LPIPS, FID, IS).  Every flag of
TestOptions stays as it is; `--hmr_model`, when it names a checkpoint of the HMR regressor, adds SSPE; `--lpips_alex` and
`--lpips_lin` together add LPIPS; `--inception` adds FID and the Inception Score."""
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
        p.add_argument('--lpips_alex', type=str, default='',
                       help="torchvision's AlexNet state_dict (features.{0,3,6,8,10}.weight / .bias); with --lpips_lin adds LPIPS")
        p.add_argument('--lpips_lin', type=str, default='',
                       help="the LPIPS v0.1 linear layers (alex.pth: lin{0..4}.model.1.weight); with --lpips_alex adds LPIPS")
        p.add_argument('--inception', type=str, default='',
                       help="torchvision's inception_v3 state_dict (<name>.conv.weight, <name>.bn.*; AuxLogits and fc are ignored); "
                            "adds fid, is and is_std over the same predictions and ground-truth frames")
