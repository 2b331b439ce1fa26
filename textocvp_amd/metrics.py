"""
Metric tracker of the evaluation step after the rollout -- mirror of the reference's
lib/metrics.py (MetricTracker :15-144, PSNR :181-212, SSIM :216-255) on the HIP metric kernel
(tocvp_psnr_ssim_f32).  The reference delegates to piqa==1.2.2 (environment.yml:26), which is not
vendored: the kernel restates piqa's published PSNR / SSIM definitions (parity with piqa itself is
unpinned; the test suite checks the kernel against an independent float64 restatement).
Frames too large for one workgroup's LDS (the ExtendedDINOSAUR family at 224 / 336) run the banded form of
the same kernel.

LPIPS (reference lib/metrics.py:259-298, piqa's LPIPS(network="alex", pretrained=True, reduction=None))
runs on csrc/lpips.hip (AlexNet features on exact fp32 MFMA + the lin head; definition in that file).
The pretrained weights are never fetched: TOCVP_LPIPS_WEIGHTS names a directory holding the two files a
reference run leaves in torch.hub's cache ($TORCH_HOME/hub/checkpoints): alexnet-owt-7be5be79.pth
(torchvision state_dict) and alex.pth (LPIPS v0.1 lin weights), or ``LPIPS(weights=(alexnet_sd, lin_sd))``
takes the two state dicts directly.  Without either, LPIPS raises NotImplementedError.
"""

import json
import os

import torch

from . import kernels as K

__all__ = ["MetricTracker", "PSNR", "SSIM", "LPIPS", "METRICS_DICT", "load_lpips_weights", "check_lpips_weights"]


class _FrameMetric:
    """ per-(sequence, frame) metric accumulated over batches; aggregate -> (mean, framewise) """

    LOWER_BETTER = False
    which = None

    def __init__(self):
        self.reset()

    def reset(self):
        self.values = []

    def _check(self, t, name):
        if t.dim() != 5:
            raise ValueError(f"{name} with {t.shape = }, but it must be (B, F, C, H, W)")

    def accumulate(self, preds, targets):
        self._check(preds, "Preds"), self._check(targets, "Targets")
        B, F, C, H, W = preds.shape
        p, s = K.psnr_ssim(preds.reshape(B * F, C, H, W), targets.reshape(B * F, C, H, W),
                           clamp01=True, want_psnr=self.which == "psnr",
                           want_ssim=self.which == "ssim")
        cur = (p if self.which == "psnr" else s).view(B, F)
        self.values.append(cur)
        return cur.mean()

    def aggregate(self):
        allv = torch.cat(self.values, dim=0)
        return float(allv.mean()), allv.mean(dim=0)


class PSNR(_FrameMetric):
    which = "psnr"


class SSIM(_FrameMetric):
    which = "ssim"

    def __init__(self, window_size=11, sigma=1.5, n_channels=3):
        if window_size != 11 or sigma != 1.5:
            raise NotImplementedError("the SSIM kernel is built for the reference's 11-tap sigma 1.5 window")
        super().__init__()


LPIPS_ALEXNET_FILE = "alexnet-owt-7be5be79.pth"
LPIPS_LIN_FILE = "alex.pth"
_ALEX_CONVS = (0, 3, 6, 8, 10)          # indices of the five convs in torchvision's alexnet().features


def check_lpips_weights(alexnet_sd, lin_sd):
    """ validate the two state dicts -> (conv weights, conv biases, lin vectors) as fp32 CPU tensors.  alexnet_sd: a
    torchvision AlexNet state_dict (classifier.* ignored); lin_sd: LPIPS v0.1 ``lin{l}.model.1.weight`` or piqa's
    ``{l}.1.weight``, each (1, C, 1, 1).  Raises ValueError naming the first missing key or wrong shape. """
    def get(sd, key, shape):
        if key not in sd:
            raise ValueError(f"LPIPS weights: missing key {key!r}")
        t = sd[key]
        if not torch.is_tensor(t) or tuple(t.shape) != shape:
            got = tuple(t.shape) if torch.is_tensor(t) else type(t).__name__
            raise ValueError(f"LPIPS weights: {key!r} has shape {got}, expected {shape}")
        return t.detach().to("cpu", torch.float32).contiguous()

    conv_w, conv_b, lin = [], [], []
    for l, (i, (ks, cin, cout)) in enumerate(zip(_ALEX_CONVS, K.LPIPS_LAYERS)):
        conv_w.append(get(alexnet_sd, f"features.{i}.weight", (cout, cin, ks, ks)))
        conv_b.append(get(alexnet_sd, f"features.{i}.bias", (cout,)))
        key = f"lin{l}.model.1.weight"
        if key not in lin_sd and f"{l}.1.weight" in lin_sd:          # piqa's renamed keys
            key = f"{l}.1.weight"
        lin.append(get(lin_sd, key, (1, cout, 1, 1)).reshape(cout))
    return conv_w, conv_b, lin


def load_lpips_weights(directory):
    """ the two files of ``directory`` (named as torch.hub caches them) -> check_lpips_weights of their contents """
    sds = []
    for name in (LPIPS_ALEXNET_FILE, LPIPS_LIN_FILE):
        path = os.path.join(directory, name)
        if not os.path.isfile(path):
            raise FileNotFoundError(f"LPIPS weights: {path} not found (TOCVP_LPIPS_WEIGHTS = {directory!r})")
        sds.append(torch.load(path, map_location="cpu", weights_only=True))
    return check_lpips_weights(*sds)


class LPIPS(_FrameMetric):
    """ piqa 1.2.2's LPIPS(network="alex", pretrained=True, reduction=None) on the HIP kernels of csrc/lpips.hip; weights
    from ``weights=(alexnet_sd, lin_sd)`` or the directory named by TOCVP_LPIPS_WEIGHTS, parsed here on the CPU and packed /
    uploaded on the first accumulate """

    LOWER_BETTER = True

    def __init__(self, network="alex", pretrained=True, reduction=None, weights=None):
        if network != "alex" or pretrained is not True or reduction is not None:
            raise NotImplementedError("LPIPS is built for network='alex', pretrained=True, reduction=None only "
                                      "(the reference's call)")
        if weights is None:
            directory = os.environ.get("TOCVP_LPIPS_WEIGHTS", "")
            if not directory:
                raise NotImplementedError(
                    "lpips needs the pretrained AlexNet + LPIPS lin weights, which are never downloaded: set "
                    f"TOCVP_LPIPS_WEIGHTS to a directory holding {LPIPS_ALEXNET_FILE} and {LPIPS_LIN_FILE} "
                    "(e.g. $TORCH_HOME/hub/checkpoints of a machine that ran the reference), or pass weights=")
            self.params = load_lpips_weights(directory)
        else:
            self.params = check_lpips_weights(*weights)
        self.packed = None
        super().__init__()

    def accumulate(self, preds, targets):
        self._check(preds, "Preds"), self._check(targets, "Targets")
        B, F, C, H, W = preds.shape
        if self.packed is None or self.packed.device != preds.device:
            self.packed = K.pack_lpips_weights(*self.params, device=preds.device)
        cur = K.lpips(preds.reshape(B * F, C, H, W), targets.reshape(B * F, C, H, W), self.packed).view(B, F)
        self.values.append(cur)
        return cur.mean()


METRICS_DICT = {"psnr": PSNR, "ssim": SSIM, "lpips": LPIPS}


class MetricTracker:
    """ same surface as the reference tracker: accumulate / aggregate / get_results / summary / save """

    def __init__(self, exp_path=None, metrics=["psnr", "ssim"]):
        if not isinstance(metrics, list):
            raise TypeError(f"'metrics' must be a list, not {type(metrics)}")
        for m in metrics:
            if m not in METRICS_DICT:
                raise NameError(f"Unknown metric = {m}. Use one of {list(METRICS_DICT)}")
        self.exp_path = exp_path
        self.metric_computers = {m: METRICS_DICT[m]() for m in metrics}
        self.reset_results()

    def reset_results(self):
        self.results = {m: None for m in self.metric_computers}
        for m in self.metric_computers.values():
            m.reset()

    def accumulate(self, preds, targets):
        for mc in self.metric_computers.values():
            mc.accumulate(preds=preds, targets=targets)

    def aggregate(self):
        for name, mc in self.metric_computers.items():
            mean, framewise = mc.aggregate()
            self.results[name] = {"mean": mean, "framewise": framewise}

    def get_results(self):
        return self.results

    def summary(self):
        for name in self.metric_computers:
            print(f"  {name}:  {round(self.results[name]['mean'], 3)}")
        return self.results

    def save_results(self, exp_path, fname):
        results_dir = os.path.join(exp_path, "results", fname)
        os.makedirs(results_dir, exist_ok=True)
        results_file = os.path.join(results_dir, "results.json")
        cur = {}
        for name, res in self.results.items():
            if res is None:
                continue
            cur[name] = {"mean": round(res["mean"], 5),
                         "framewise": [round(r, 5) for r in res["framewise"].cpu().tolist()]}
        if os.path.exists(results_file):
            with open(results_file) as f:
                for k, v in json.load(f).items():
                    cur.setdefault(k, v)
        with open(results_file, "w") as f:
            json.dump(cur, f)
