"""
LPIPS on the HIP kernels (csrc/lpips.hip) against the float64 restatement of tests/test_lpips_cpu.py, the metric tracker
with all three of the reference evaluators' metrics (base/baseEvaluator.py:56-59), and PSNR / SSIM on frames above the
LDS limit of the one-workgroup metric kernel (the banded form of csrc/metrics.hip).
"""

import json

import pytest
import torch
import torch.nn.functional as F

from oracle import metrics_oracle as MO
from test_lpips_cpu import SCALE, SHIFT, lpips_ref, synth_lpips_state_dicts, write_weight_files
from textocvp_amd import kernels as K
from textocvp_amd import metrics as M

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _frames(n, H, W, seed):
    """ pairs straying outside [0, 1] on both sides (the fused clamp) """
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, 3, H, W, generator=g) * 1.3 - 0.15
    y = (0.6 * x + 0.4 * torch.rand(n, 3, H, W, generator=g) + 0.05 * torch.randn(n, 3, H, W, generator=g))
    return x, y.clamp(-0.2, 1.2)


_CACHE = {}


def _weights(seed=0, bias_shift=None):
    key = (seed, str(bias_shift))
    if key not in _CACHE:
        alex, lin = synth_lpips_state_dicts(seed=seed, bias_shift=bias_shift)
        params = M.check_lpips_weights(alex, lin)
        _CACHE[key] = (alex, lin, params, K.pack_lpips_weights(*params, device=DEV))
    return _CACHE[key]


@pytest.mark.parametrize("N,H,W", [(4, 64, 64), (2, 224, 224), (2, 336, 336), (3, 65, 97), (3, 31, 31)])
def test_lpips_against_fp64(N, H, W):
    _, _, params, packed = _weights()
    x, y = _frames(N, H, W, seed=H * 7 + W)
    got = K.lpips(x.to(DEV), y.to(DEV), packed).cpu().double()
    ref = lpips_ref(x, y, *params)
    err = float((got - ref).abs().max())
    print(f"LPIPS {N}x{H}x{W}: max |kernel - fp64| = {err:.2e} (values {ref.min():.4f} .. {ref.max():.4f})")
    assert bool(torch.isfinite(got).all()) and err < 1e-5


def test_lpips_layers_alone():
    _, _, (cw, cb, _), packed = _weights()
    x, y = _frames(2, 67, 61, seed=11)
    # conv1: stride 4, NCHW in from two base pointers, clamp + scaling fused, NHWC out
    c1 = K.lpips_conv(0, x.to(DEV), packed, x2=y.to(DEV))
    s = (torch.cat([x, y]).double().clamp(0, 1) - SHIFT) / SCALE
    r1 = F.relu(F.conv2d(s, cw[0].double(), cb[0].double(), stride=4, padding=2))
    assert c1.shape == (4, 16, 14, 64)
    e1 = float((c1.cpu().double().permute(0, 3, 1, 2) - r1).abs().max())
    assert e1 < 2e-5 * max(1.0, float(r1.abs().max())), e1
    # the pooled input of conv2: bitwise max of the kernel's conv1, and against the fp64 chain
    p1 = K.lpips_maxpool(c1)
    assert torch.equal(p1.permute(0, 3, 1, 2), F.max_pool2d(c1.permute(0, 3, 1, 2), 3, 2))
    rp = F.max_pool2d(r1, 3, 2)
    assert float((p1.cpu().double().permute(0, 3, 1, 2) - rp).abs().max()) < 2e-5 * max(1.0, float(rp.abs().max()))
    # conv5 alone on a non-negative NHWC map
    g = torch.Generator().manual_seed(5)
    f = torch.relu(torch.randn(3, 9, 7, 256, generator=g))
    c5 = K.lpips_conv(4, f.to(DEV), packed)
    r5 = F.relu(F.conv2d(f.double().permute(0, 3, 1, 2), cw[4].double(), cb[4].double(), padding=1))
    e5 = float((c5.cpu().double().permute(0, 3, 1, 2) - r5).abs().max())
    assert e5 < 2e-5 * max(1.0, float(r5.abs().max())), e5


def test_lpips_exact_identities():
    _, _, _, packed = _weights()
    x, y = (t.to(DEV) for t in _frames(5, 64, 64, seed=3))
    assert torch.equal(K.lpips(x, x, packed), torch.zeros(5, device=DEV))
    a, b = K.lpips(x, y, packed), K.lpips(y, x, packed)
    assert torch.equal(a, b)
    assert torch.equal(a, K.lpips(x, y, packed))
    assert bool((a > 0).all())


def test_lpips_all_zero_feature_vectors():
    # conv5 entirely below zero (every tap-5 vector is zero), half of conv3's channels, a quarter of conv1's
    shift = {0: (-1e3, 0.25), 2: (-1e3, 0.5), 4: (-1e3, 1.0)}
    _, _, params, packed = _weights(seed=6, bias_shift=shift)
    x, y = _frames(3, 64, 64, seed=8)
    c5 = K.lpips_conv(4, torch.relu(torch.randn(1, 3, 3, 256)).to(DEV), packed)
    assert float(c5.abs().max()) == 0.0
    got = K.lpips(x.to(DEV), y.to(DEV), packed).cpu().double()
    ref = lpips_ref(x, y, *params)
    assert bool(torch.isfinite(got).all()) and float((got - ref).abs().max()) < 1e-5


def test_lpips_chunking_matches_single_pairs():
    _, _, _, packed = _weights()
    x, y = (t.to(DEV) for t in _frames(7, 64, 64, seed=9))
    limit = K.lpips_ws_bytes(3, 64, 64)                 # chunks of 3, 3, 1 pairs
    got = K.lpips(x, y, packed, max_ws_bytes=limit)
    single = torch.cat([K.lpips(x[i:i + 1], y[i:i + 1], packed) for i in range(7)])
    assert torch.equal(got, single)
    assert torch.equal(got, K.lpips(x, y, packed))


@pytest.mark.parametrize("S", [64, 224])
def test_tracker_with_lpips(tmp_path, monkeypatch, S):
    alex, lin, _, packed = _weights()
    monkeypatch.setenv("TOCVP_LPIPS_WEIGHTS", write_weight_files(tmp_path, alex, lin))
    B, Fr = 2, 3
    mt = M.MetricTracker(metrics=["psnr", "ssim", "lpips"])
    a, b = _frames(B * Fr, S, S, seed=S)
    a, b = a.view(B, Fr, 3, S, S).to(DEV), b.view(B, Fr, 3, S, S).to(DEV)
    mt.accumulate(a, b)
    mt.accumulate(b, a)
    mt.aggregate()
    res = mt.get_results()
    assert set(res) == {"psnr", "ssim", "lpips"}
    direct = torch.cat([K.lpips(a.reshape(-1, 3, S, S), b.reshape(-1, 3, S, S), packed),
                        K.lpips(b.reshape(-1, 3, S, S), a.reshape(-1, 3, S, S), packed)]).view(2 * B, Fr)
    assert torch.equal(torch.cat(mt.metric_computers["lpips"].values), direct)
    assert res["lpips"]["framewise"].shape == (Fr,)
    assert abs(res["lpips"]["mean"] - float(direct.mean())) < 1e-6
    p, s = K.psnr_ssim(a.reshape(-1, 3, S, S), b.reshape(-1, 3, S, S))
    assert torch.equal(mt.metric_computers["ssim"].values[0], s.view(B, Fr))
    mt.save_results(str(tmp_path), "r")
    saved = json.load(open(tmp_path / "results" / "r" / "results.json"))
    assert set(saved) == {"psnr", "ssim", "lpips"} and len(saved["lpips"]["framewise"]) == Fr


@pytest.mark.parametrize("N,H,W", [(3, 144, 144), (2, 224, 224), (2, 336, 336), (2, 300, 157)])
def test_psnr_ssim_large_frames(N, H, W):
    """ the banded metric kernel (frames above the one-workgroup LDS limit); 224, 336 and 300 leave a partial last band """
    x, y = _frames(N, H, W, seed=H + W)
    y[0] = x[0]
    p, s = K.psnr_ssim(x.to(DEV), y.to(DEV), clamp01=True)
    xc, yc = x.clamp(0, 1), y.clamp(0, 1)
    assert float((p.cpu().double() - MO.psnr(xc.double(), yc.double())).abs().max()) < 2e-6 * 80
    assert float((s.cpu().double() - MO.ssim(xc, yc).double()).abs().max()) < 2e-5
    assert abs(s[0].item() - 1.0) < 1e-5 and abs(p[0].item() - 80.0) < 1e-3


@torch.no_grad()
def test_decomp_eval_dinosaur_224_three_metrics(tmp_path, monkeypatch):
    from textocvp_amd import synth
    from textocvp_amd.evaluator import forward_eval_decomp
    from textocvp_amd.setup_model import default_dinosaur_params, setup_model
    alex, lin, _, packed = _weights()
    monkeypatch.setenv("TOCVP_LPIPS_WEIGHTS", write_weight_files(tmp_path, alex, lin))
    S, Kk = 224, 24
    model = setup_model(default_dinosaur_params(num_slots=Kk, img_size=S)).eval()
    synth.fill_module_(model, prefix="dino.")
    model = model.to(DEV)
    videos = synth.synth_videos(1, 3, height=S, width=S, seed=5).to(DEV)
    tracker = M.MetricTracker(metrics=["psnr", "ssim", "lpips"])
    out = forward_eval_decomp(model, videos, metric_tracker=tracker, init_noise=synth.synth_noise(1, Kk, 128, seed=6).to(DEV))
    tracker.aggregate()
    res = tracker.get_results()
    for name in ("psnr", "ssim", "lpips"):
        assert res[name]["framewise"].shape == (3,) and bool(torch.isfinite(res[name]["framewise"]).all()), name
    rc = out["recons_clamped"].reshape(3, 3, S, S)
    v = videos.reshape(3, 3, S, S)
    p, s = K.psnr_ssim(rc, v)
    assert torch.equal(tracker.metric_computers["psnr"].values[0].view(-1), p)
    assert torch.equal(tracker.metric_computers["ssim"].values[0].view(-1), s)
    assert torch.equal(tracker.metric_computers["lpips"].values[0].view(-1), K.lpips(rc, v, packed))
