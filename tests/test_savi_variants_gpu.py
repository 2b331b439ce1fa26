"""
SAVi variants on the MI355X: the kernel-3 / 5 / 7 convolutions (with and without the fused nearest x2 upsampling) against
fp64 torch, the collapsed layer 0 and the tail at widths 32 / 128, and every variant against the fixtures the
reference produced (tests/golden/make_golden_savi_variants.py) at the suite's bars, in the default arithmetic, in fp32
and after a range fallback.
"""

import copy
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, max_abs
from textocvp_amd import kernels as K
from textocvp_amd import synth
from textocvp_amd.evaluator import GraphedEval, forward_eval
from textocvp_amd.setup_model import default_exp_params, setup_model, setup_predictor

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VARIANTS = ("up2", "k3", "bn_up2_128", "k7_mixed")
WIDTHS = (32, 64, 128)
# (n, SH, SW) source sizes: square 8 x 8, non-square, wider than one 32-pixel tile, narrow 16 x 16
SHAPES = ((3, 8, 8), (2, 16, 24), (2, 8, 40), (2, 16, 16))


def _ref_conv(x, w, scale, shift, k, relu, up):
    """ fp64 CPU reference on NHWC fp32 input """
    xd = x.double().cpu().permute(0, 3, 1, 2)
    if up:
        xd = F.interpolate(xd, scale_factor=2, mode="nearest")
    y = F.conv2d(xd, w.double().cpu(), padding=k // 2)
    if scale is not None:
        y = y * scale.double().cpu()[None, :, None, None]
    y = y + shift.double().cpu()[None, :, None, None]
    if relu:
        y = y.clamp_min(0)
    return y.permute(0, 2, 3, 1)


def _grid():
    cases, i = [], 0
    for k in (3, 5, 7):
        for up in (False, True):
            for cin in WIDTHS:
                for cout in WIDTHS:
                    cases.append((k, up, cin, cout, SHAPES[i % len(SHAPES)], i % 2 == 0, i % 3 != 0))
                    i += 1
    return cases


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
@pytest.mark.parametrize("k,up,cin,cout,shape,relu,with_scale", _grid())
def test_convk_against_fp64(precision, k, up, cin, cout, shape, relu, with_scale):
    n, SH, SW = shape
    g = torch.Generator().manual_seed(k * 1000 + cin + cout + up)
    x = torch.randn((n, SH, SW, cin), generator=g).to(DEV)
    w = (torch.rand((cout, cin, k, k), generator=g) * 2 - 1).mul_((cin * k * k) ** -0.5).to(DEV)
    scale = (0.5 + torch.rand(cout, generator=g)).to(DEV) if with_scale else None
    shift = (torch.rand(cout, generator=g) - 0.5).to(DEV)
    if precision == "f16x3" and up:
        wk = K.pack_conv_up2_weights(w)
    else:
        wk = K.pack_conv_weights(w)
    y = K.convk(x, wk, scale, shift, k, relu=relu, upsample2=up, precision=precision)
    torch.cuda.synchronize()
    ref = _ref_conv(x, w, scale, shift, k, relu, up)
    assert y.shape == ref.shape
    err = (y.double().cpu() - ref).abs().max().item()
    bar = 3e-6 * ref.abs().max().item()
    assert err <= bar, f"max|err| {err:.3g} > {bar:.3g}"


def test_convk_refuses_other_widths():
    x = torch.zeros((1, 8, 8, 48), device=DEV)
    wp = torch.zeros((9, 32, 48), device=DEV)
    with pytest.raises(NotImplementedError):
        K.convk(x, wp, None, torch.zeros(32, device=DEV), 3)
    # the C-ABI itself refuses as well
    rc = K.lib().tocvp_convk_f32(K._ptr(x), K._ptr(wp), None, K._ptr(wp), K._ptr(x), 1, 8, 8, 48, 32, 3, 1, 0, None)
    assert rc != 0


@pytest.mark.parametrize("k,H,W,C,D", [(3, 8, 8, 64, 128), (5, 16, 8, 32, 64), (7, 8, 16, 128, 128)])
def test_collapsed_layer0_against_broadcast_conv(k, H, W, C, D):
    g = torch.Generator().manual_seed(k)
    n = 5
    slots = torch.randn((n, D), generator=g)
    pos = torch.randn((H, W, D), generator=g) * 0.5
    w = (torch.rand((C, D, k, k), generator=g) * 2 - 1) * (D * k * k) ** -0.5
    scale, shift = 0.5 + torch.rand(C, generator=g), torch.rand(C, generator=g) - 0.5
    wd = w.to(DEV)
    zero = torch.zeros(C, device=DEV)
    cpos = K.convk(pos[None].to(DEV).contiguous(), K.pack_conv_weights(wd), None, zero, k, relu=False,
                   precision="fp32")[0].contiguous()
    ts = K.dec_tapsum_k(wd)
    S = (slots.double() @ ts.double().cpu().reshape(k * k * C, D).T).float().reshape(n, k * k, C).to(DEV)
    y = K.dec_layer0_expand(cpos, S.contiguous(), scale.to(DEV), shift.to(DEV), k, relu=True)
    torch.cuda.synchronize()
    bcast = slots.double()[:, None, None, :] + pos.double()[None]                     # (n, H, W, D): explicit
    ref = F.conv2d(bcast.permute(0, 3, 1, 2), w.double(), padding=k // 2)
    ref = (ref * scale.double()[None, :, None, None] + shift.double()[None, :, None, None]).clamp_min(0)
    ref = ref.permute(0, 2, 3, 1)
    err = (y.double().cpu() - ref).abs().max().item()
    assert err <= 3e-6 * ref.abs().max().item(), err


@pytest.mark.parametrize("C", [32, 128])
def test_generic_tail_widths(C):
    g = torch.Generator().manual_seed(C)
    Fr, Ks, H, W = 2, 5, 16, 32
    x = torch.rand((Fr * Ks, H, W, C), generator=g)
    w = (torch.rand((4, C, 3, 3), generator=g) * 2 - 1) * (C * 9) ** -0.5
    b = torch.rand(4, generator=g) - 0.5
    imgs, recons, masks = K.dec_tail(x.to(DEV), w.to(DEV), b.to(DEV), Fr, Ks)
    torch.cuda.synchronize()
    y = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), b.double(), padding=1).reshape(Fr, Ks, 4, H, W)
    rc, al = y[:, :, :3], torch.softmax(y[:, :, 3:], dim=1)
    assert max_abs(recons.cpu(), rc) < 2e-6
    assert max_abs(masks.cpu(), al) < 2e-6
    assert max_abs(imgs.cpu(), (rc * al).sum(1)) < 2e-6


# ---- variants against the reference's fixtures ------------------------------------------------------------------------
def manifest(tag):
    with open(os.path.join(GOLDEN, f"state_dict_manifest_savi_{tag}.json")) as f:
        return json.load(f)


def build(tag, precision=None):
    model_params = copy.deepcopy(manifest(tag)["model_params"])
    exp = default_exp_params(num_slots=model_params["num_slots"], num_context=1, num_preds=2)
    exp["model"]["model_params"] = model_params
    savi = setup_model(exp["model"]).eval()
    pred = setup_predictor(exp).eval()
    synth.fill_module_(savi, prefix="savi.")
    synth.fill_batchnorm_stats_(savi, prefix="savi.")
    synth.fill_module_(pred, prefix="pred.")
    if precision == "fp32":
        savi.decoder.generic_precision = "fp32"
        savi.encoder.conv_precision = "fp32"
    return savi.to(DEV), pred.to(DEV)


def image_size(tag):
    return tuple(manifest(tag)["model_params"]["encoder"]["encoder_params"]["resolution"])


def check_units(tag, savi):
    g = load_golden(f"savi_{tag}.npz")
    H, W = image_size(tag)
    step, fs, im = int(g["sub_step"]), int(g["feat_step"]), int(g["img_step"])
    with torch.no_grad():
        imgs = synth.synth_tensor(f"variants.{tag}.imgs", (2, 3, H, W), "unit").to(DEV)
        feats = savi.encode(imgs)
        assert tuple(feats.shape) == (2, H * W, 128)
        assert max_abs(feats[:, ::fs].cpu(), g["encoder_feats_sub"]) < 5e-5
        dslots = synth.synth_tensor(f"variants.{tag}.dec_slots", (2, 7, 128), "normal").to(DEV)
        out = savi(mode="decode", slots=dslots)
    assert tuple(out["recons_imgs"].shape) == (2, 3, H, W)
    assert max_abs(out["recons_imgs"][..., ::im, ::im].cpu(), g["dec_recons_imgs_sub"]) < 5e-5
    assert max_abs(out["recons"][..., ::step, ::step].cpu(), g["dec_recons_sub"]) < 5e-5
    assert max_abs(out["masks"][..., ::step, ::step].cpu(), g["dec_masks_sub"]) < 1e-4
    assert np.array_equal(out["masks"].argmax(dim=1).to(torch.uint8).cpu().numpy(), g["dec_masks_argmax"])


def e2e_inputs(tag):
    H, W = image_size(tag)
    videos = synth.synth_videos(1, 3, height=H, width=W, seed=0).to(DEV)
    tokens, lengths = synth.synth_captions(1, max_len=10, seed=0)
    noise = synth.synth_noise(1, 7, 128, seed=1).to(DEV)
    return videos, dict(caption_tokens=tokens.to(DEV), caption_lengths=lengths.to(DEV), init_noise=noise)


def check_e2e(tag, savi, pred):
    g = load_golden(f"savi_{tag}.npz")
    videos, kw = e2e_inputs(tag)
    with torch.no_grad():
        out = forward_eval(savi, pred, videos, 1, 2, **kw)
    torch.cuda.synchronize()
    assert max_abs(out["slot_history"].cpu(), g["e2e_slot_history"]) < 1e-4
    assert max_abs(out["pred_slots"].cpu(), g["e2e_pred_slots"]) < 1e-4
    im = int(g["img_step"])
    assert max_abs(out["pred_imgs"][..., ::im, ::im].cpu(), g["e2e_pred_imgs_sub"]) < 1e-4
    am = out["masks"].reshape(-1, *out["masks"].shape[-4:]).argmax(dim=1).to(torch.uint8).cpu().numpy()
    assert np.array_equal(am, g["e2e_masks_argmax"].reshape(am.shape))


@pytest.mark.parametrize("precision", [None, "fp32"])
@pytest.mark.parametrize("tag", VARIANTS)
def test_variant_against_reference_fixture(tag, precision):
    savi, pred = build(tag, precision)
    assert savi.decoder.generic
    check_units(tag, savi)
    if tag in ("up2", "bn_up2_128"):
        check_e2e(tag, savi, pred)


@pytest.mark.parametrize("tag", ["up2", "bn_up2_128"])
def test_forced_range_fallback_ends_on_fp32(tag, monkeypatch):
    savi, _ = build(tag)
    if savi.decoder.generic_precision != "f16x3":
        pytest.skip("arithmetic already fp32 (TOCVP_PRECISION=fp32)")
    dslots = synth.synth_tensor(f"variants.{tag}.dec_slots", (2, 7, 128), "normal").to(DEV)
    monkeypatch.setattr(K, "F16X3_ACT_RANGE", 1e-3)             # every f16x3 operand now counts as out of range
    with torch.no_grad(), K.check_range(True), pytest.raises(K.TocvpRangeError) as err:
        savi.decode(dslots)
    mod, attr = err.value.owner
    assert mod is savi.decoder and attr == "generic_precision"
    setattr(mod, attr, type(mod).range_fallbacks[attr][getattr(mod, attr)])
    assert savi.decoder.generic_precision == "fp32"
    monkeypatch.undo()
    check_units(tag, savi)


def test_graphed_eval_replay_is_bit_identical_on_up2():
    savi, pred = build("up2")
    videos, kw = e2e_inputs("up2")
    with torch.no_grad():
        eager = forward_eval(savi, pred, videos, 1, 2, overlap_decode=False, **kw)["pred_imgs"].clone()
        graphed = GraphedEval(savi, pred, 1, 2)
        for _ in range(2):
            assert torch.equal(graphed(videos, **kw)["pred_imgs"], eager)
