"""
LPIPS without a GPU: the weight loader behind TOCVP_LPIPS_WEIGHTS / LPIPS(weights=...), the refusal without weights, and
the float64 restatement of the metric (reference lib/metrics.py:259-298, piqa 1.2.2 LPIPS(network="alex"), as written at
the top of textocvp_amd/csrc/lpips.hip) that tests/test_lpips_gpu.py checks the HIP kernels against.
"""

import pytest
import torch
import torch.nn.functional as F

from textocvp_amd import metrics as M

LAYERS = ((11, 3, 64), (5, 64, 192), (3, 192, 384), (3, 384, 256), (3, 256, 256))   # (kernel, Cin, Cout)
ALEX_IDX = (0, 3, 6, 8, 10)
SHIFT = torch.tensor([0.485, 0.456, 0.406], dtype=torch.float64).view(1, 3, 1, 1)
SCALE = torch.tensor([0.229, 0.224, 0.225], dtype=torch.float64).view(1, 3, 1, 1)


def synth_lpips_state_dicts(seed=0, piqa_keys=False, bias_shift=None):
    """ He-scaled AlexNet convs (+ classifier entries, which the loader ignores) and non-negative lin weights.
    bias_shift: {layer: (value, fraction of channels)} pushes biases down so that those channels are zero after ReLU """
    g = torch.Generator().manual_seed(seed)
    alex = {}
    for l, (i, (ks, cin, cout)) in enumerate(zip(ALEX_IDX, LAYERS)):
        alex[f"features.{i}.weight"] = torch.randn(cout, cin, ks, ks, generator=g) * (2.0 / (cin * ks * ks)) ** 0.5
        b = torch.randn(cout, generator=g) * 0.05
        if bias_shift and l in bias_shift:
            v, frac = bias_shift[l]
            b[:int(round(frac * cout))] = v
        alex[f"features.{i}.bias"] = b
    alex["classifier.1.weight"] = torch.zeros(4, 9216)
    alex["classifier.1.bias"] = torch.zeros(4)
    lin = {}
    for l, (_, _, cout) in enumerate(LAYERS):
        key = f"{l}.1.weight" if piqa_keys else f"lin{l}.model.1.weight"
        lin[key] = torch.rand(1, cout, 1, 1, generator=g) * 0.2
    return alex, lin


def write_weight_files(directory, alex, lin):
    torch.save(alex, str(directory / M.LPIPS_ALEXNET_FILE))
    torch.save(lin, str(directory / M.LPIPS_LIN_FILE))
    return str(directory)


def lpips_ref(x, y, conv_w, conv_b, lin):
    """ float64 restatement: x, y (N, 3, H, W) -> (N,).  Both inputs clamped to [0, 1] (the metric step's clamp). """
    def feats(t):
        t = (t.double().clamp(0, 1) - SHIFT) / SCALE
        taps = []
        for l, (w, b) in enumerate(zip(conv_w, conv_b)):
            stride, pad = (4, 2) if l == 0 else (1, w.shape[-1] // 2)
            t = F.relu(F.conv2d(t, w.double(), b.double(), stride=stride, padding=pad))
            taps.append(t)
            if l < 2:
                t = F.max_pool2d(t, 3, 2)
        return taps

    total = torch.zeros(x.shape[0], dtype=torch.float64)
    for a, b, w in zip(feats(x), feats(y), lin):
        a = a / (a.norm(dim=1, keepdim=True) + 1e-10)
        b = b / (b.norm(dim=1, keepdim=True) + 1e-10)
        total = total + ((a - b) ** 2 * w.double().view(1, -1, 1, 1)).sum(dim=1).mean(dim=(1, 2))
    return total


@pytest.mark.parametrize("piqa_keys", [False, True])
def test_weight_files_load_with_both_key_spellings(tmp_path, monkeypatch, piqa_keys):
    alex, lin = synth_lpips_state_dicts(seed=1, piqa_keys=piqa_keys)
    d = write_weight_files(tmp_path, alex, lin)
    conv_w, conv_b, lins = M.load_lpips_weights(d)
    assert [tuple(w.shape) for w in conv_w] == [(co, ci, k, k) for k, ci, co in LAYERS]
    assert [tuple(v.shape) for v in lins] == [(co,) for _, _, co in LAYERS]
    for l, i in enumerate(ALEX_IDX):
        assert torch.equal(conv_w[l], alex[f"features.{i}.weight"])
        assert torch.equal(conv_b[l], alex[f"features.{i}.bias"])
        key = f"{l}.1.weight" if piqa_keys else f"lin{l}.model.1.weight"
        assert torch.equal(lins[l], lin[key].reshape(-1))
    monkeypatch.setenv("TOCVP_LPIPS_WEIGHTS", d)
    metric = M.LPIPS()                          # the knob path: parsed on the CPU, nothing uploaded yet
    assert metric.LOWER_BETTER and metric.packed is None
    assert torch.equal(metric.params[0][2], conv_w[2])
    assert M.LPIPS(weights=(alex, lin)).packed is None


def test_bad_weights_name_the_key(tmp_path):
    alex, lin = synth_lpips_state_dicts(seed=2)
    bad = dict(alex)
    del bad["features.6.bias"]
    with pytest.raises(ValueError, match=r"features\.6\.bias"):
        M.check_lpips_weights(bad, lin)
    bad = dict(alex)
    bad["features.3.weight"] = torch.zeros(192, 64, 3, 3)
    with pytest.raises(ValueError, match=r"features\.3\.weight.*\(192, 64, 5, 5\)"):
        M.check_lpips_weights(bad, lin)
    bad_lin = dict(lin)
    del bad_lin["lin4.model.1.weight"]
    with pytest.raises(ValueError, match=r"lin4\.model\.1\.weight"):
        M.check_lpips_weights(alex, bad_lin)
    bad_lin = dict(lin)
    bad_lin["lin1.model.1.weight"] = torch.zeros(1, 64, 1, 1)
    with pytest.raises(ValueError, match=r"lin1\.model\.1\.weight"):
        M.check_lpips_weights(alex, bad_lin)
    # the same through the files
    del bad["features.3.weight"]
    with pytest.raises(ValueError, match=r"features\.3\.weight"):
        M.load_lpips_weights(write_weight_files(tmp_path, bad, lin))


def test_refusal_without_weights(monkeypatch):
    monkeypatch.delenv("TOCVP_LPIPS_WEIGHTS", raising=False)
    with pytest.raises(NotImplementedError, match="TOCVP_LPIPS_WEIGHTS"):
        M.MetricTracker(metrics=["lpips"])
    with pytest.raises(NotImplementedError):
        M.LPIPS(weights=synth_lpips_state_dicts(), network="vgg")
    with pytest.raises(NotImplementedError):
        M.LPIPS(weights=synth_lpips_state_dicts(), reduction="mean")
    assert M.METRICS_DICT["lpips"] is M.LPIPS
    assert list(M.MetricTracker().metric_computers) == ["psnr", "ssim"]      # default list unchanged


def _ref_params(seed):
    alex, lin = synth_lpips_state_dicts(seed=seed)
    return M.check_lpips_weights(alex, lin)


def test_restatement_identity_and_batching():
    params = _ref_params(3)
    g = torch.Generator().manual_seed(4)
    x = torch.rand(3, 3, 40, 47, generator=g, dtype=torch.float64) * 1.2 - 0.1
    y = torch.rand(3, 3, 40, 47, generator=g, dtype=torch.float64)
    assert torch.equal(lpips_ref(x, x, *params), torch.zeros(3, dtype=torch.float64))
    d = lpips_ref(x, y, *params)
    assert bool((d > 0).all())
    one_by_one = torch.cat([lpips_ref(x[i:i + 1], y[i:i + 1], *params) for i in range(3)])
    assert torch.allclose(d, one_by_one, rtol=0, atol=1e-12)
