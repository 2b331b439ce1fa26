"""
Predictor training on frozen SAVi variants on the MI355X: the data gradient of the variant convolutions (k 3 / 5 / 7, with
and without the x2 upsampling, every width pairing), the tail backward at widths 32 / 64 / 128 and the layer-0 class
reduce against fp64, GenericDecoderLoss against torch.autograd of a reference-form decoder written here (F.conv2d,
nearest F.interpolate, eval F.batch_norm, softmax over the slots), and the whole training step: selection, graph replay
of the decoder backward, the range fallback.
"""

import copy
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from textocvp_amd import kernels as K
from textocvp_amd import synth
from textocvp_amd.setup_model import default_exp_params, setup_model, setup_predictor

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VARIANTS = ("up2", "k3", "bn_up2_128", "k7_mixed")
WIDTHS = (32, 64, 128)
# (n, H, W) of dx: square 8 x 8 and 16 x 16 (the up2 sources), odd 7 x 7 / 9 x 9, partial tiles in both directions
SHAPES = ((2, 8, 8), (1, 16, 16), (2, 7, 7), (1, 9, 9), (1, 12, 40))


def _lib():
    return K.lib()


def _s():
    return torch.cuda.current_stream().cuda_stream


# ---- data gradient ------------------------------------------------------------------------------------------------
def _dgrad_case(k, up2, cg, cout, shape, seed):
    n, H, W = shape
    gen = torch.Generator().manual_seed(seed)
    GH, GW = (2 * H, 2 * W) if up2 else (H, W)
    # image-loss scale: ~1e-8 gradients
    g = torch.randn((n, GH, GW, cg), generator=gen) * 1e-8
    w = (torch.rand((cg, cout, k, k), generator=gen) * 2 - 1) * (cout * k * k) ** -0.5
    scale = 0.5 + torch.rand(cg, generator=gen)
    gate = torch.randn((n, H, W, cout), generator=gen)
    return g, w, scale, gate


def _dgrad_ref(g, w, scale, k, up2, H, W):
    """ fp64 autograd of x -> conv2d([nearest x2] x) * scale, NHWC in and out """
    n, cout = g.shape[0], w.shape[1]
    x = torch.zeros((n, cout, H, W), dtype=torch.float64, requires_grad=True)
    u = F.interpolate(x, scale_factor=2, mode="nearest") if up2 else x
    y = F.conv2d(u, w.double(), padding=k // 2) * scale.double()[None, :, None, None]
    (dx,) = torch.autograd.grad(y, x, g.double().permute(0, 3, 1, 2))
    return dx.permute(0, 2, 3, 1)


def _grid():
    cases, i = [], 0
    for k in (3, 5, 7):
        for up2 in (False, True):
            for cg in WIDTHS:
                for cout in WIDTHS:
                    cases.append((k, up2, cg, cout, SHAPES[i % len(SHAPES)]))
                    i += 1
    return cases


def _raw_dgrad(g, wsplit, gate, dx, k, up2):
    n, H, W, cout = dx.shape
    return _lib().tocvp_convk_dgrad_bf16x3_f32(g.data_ptr(), wsplit.data_ptr(), K._ptr(gate), dx.data_ptr(), n, H, W,
                                               g.shape[-1], cout, k, int(up2), _s())


@pytest.mark.parametrize("k,up2,cg,cout,shape", _grid())
def test_convk_dgrad_matches_fp64(k, up2, cg, cout, shape):
    n, H, W = shape
    g, w, scale, gate = _dgrad_case(k, up2, cg, cout, shape, seed=31 * k + cg + 7 * cout + up2)
    ref = _dgrad_ref(g, w, scale, k, up2, H, W)
    gd, gated = g.to(DEV), gate.to(DEV)
    wsplit = K.pack_convk_dgrad_weights(w.to(DEV), scale.to(DEV), up2=up2)
    # ungated through the wrapper
    dx = K.convk_dgrad(gd, wsplit, (H, W), k, up2=up2)
    torch.cuda.synchronize()
    err = (dx.double().cpu() - ref).abs().max().item() / ref.abs().max().item()
    assert err < 1e-4, err
    # gated, into a NaN-prefilled output: fully overwritten, exact zeros where the gate is off, same bits twice
    outs = []
    for _ in range(2):
        o = torch.full((n, H, W, cout), float("nan"), device=DEV)
        assert _raw_dgrad(gd, wsplit, gated, o, k, up2) == 0
        outs.append(o)
    torch.cuda.synchronize()
    o = outs[0].cpu()
    assert torch.isfinite(o).all()
    off = gate <= 0
    assert (o[off] == 0).all()
    assert torch.equal(o[~off], dx.cpu()[~off])
    assert torch.equal(outs[0], outs[1])


def test_convk_dgrad_rejects_bad_arguments():
    n, H, W = 1, 8, 8
    g = torch.zeros((n, H, W, 64), device=DEV)
    wsplit = K.pack_convk_dgrad_weights(torch.zeros((64, 64, 5, 5), device=DEV))
    sentinel = torch.full((n * H * W * 64 + 4,), 7.0, device=DEV)
    dx = sentinel[:n * H * W * 64]
    L, s = _lib(), _s()
    bad = [
        (g.data_ptr(), wsplit.data_ptr(), None, dx.data_ptr(), n, H, W, 48, 64, 5, 0),     # width 48
        (g.data_ptr(), wsplit.data_ptr(), None, dx.data_ptr(), n, H, W, 64, 96, 5, 0),     # width 96
        (g.data_ptr(), wsplit.data_ptr(), None, dx.data_ptr(), n, H, W, 64, 64, 4, 0),     # even kernel
        (g.data_ptr(), wsplit.data_ptr(), None, dx.data_ptr(), n, H, W, 64, 64, 9, 0),     # kernel 9
        (g.data_ptr(), wsplit.data_ptr(), None, dx.data_ptr(), n, H, W, 64, 64, 5, 2),     # up2 flag
        (None, wsplit.data_ptr(), None, dx.data_ptr(), n, H, W, 64, 64, 5, 0),             # null input
        (g.data_ptr(), None, None, dx.data_ptr(), n, H, W, 64, 64, 5, 0),                   # null weights
        (g.data_ptr(), wsplit.data_ptr(), None, None, n, H, W, 64, 64, 5, 0),               # null output
        (g.data_ptr(), wsplit.data_ptr(), None, dx.data_ptr(), -1, H, W, 64, 64, 5, 0),    # negative count
        (g.data_ptr(), wsplit.data_ptr(), None, dx.data_ptr(), n, 0, W, 64, 64, 5, 0),     # empty image
        (g.data_ptr() + 4, wsplit.data_ptr(), None, dx.data_ptr(), n, H, W, 64, 64, 5, 0),  # misaligned
    ]
    for args in bad:
        assert L.tocvp_convk_dgrad_bf16x3_f32(*args, s) != 0, args
    torch.cuda.synchronize()
    assert (sentinel == 7.0).all()
    with pytest.raises(NotImplementedError):
        K.convk_dgrad(torch.zeros((1, 8, 8, 48), device=DEV), wsplit, (8, 8), 5)


# ---- tail backward and layer-0 class reduce -----------------------------------------------------------------------
@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("shape", [(3, 8, 8), (2, 7, 9), (1, 16, 16), (1, 64, 64)])
def test_tail_backward_wide_matches_fp64(C, shape):
    n, H, W = shape
    gen = torch.Generator().manual_seed(C + H * 3 + W)
    dy = torch.randn((n, H, W, 4), generator=gen) * 1e-6
    w = torch.randn((4, C, 3, 3), generator=gen) * 0.1
    act = torch.randn((n, H, W, C), generator=gen).clamp_min(0)
    ref = F.conv_transpose2d(dy.double().permute(0, 3, 1, 2), w.double(), padding=1).permute(0, 2, 3, 1)
    ref = torch.where(act > 0, ref, torch.zeros_like(ref))
    dyd, wd, actd = dy.to(DEV), w.to(DEV), act.to(DEV)
    got = K.conv3x3_t4w(dyd, wd, actd)
    got2 = K.conv3x3_t4w(dyd, wd, actd)
    torch.cuda.synchronize()
    err = (got.double().cpu() - ref).abs().max().item() / ref.abs().max().item()
    assert err < 1e-5, err
    assert (got.cpu()[act <= 0] == 0).all() and torch.equal(got, got2)
    if C <= 64 and W % 4 == 0:                                   # the shipped entry's range: the same sums
        old = torch.empty_like(got)
        K._check(_lib().tocvp_conv3x3_t4_f32(dyd.data_ptr(), wd.data_ptr(), actd.data_ptr(), old.data_ptr(), n, H, W, C,
                                             _s()), "t4")
        assert torch.equal(old, got)


def _class_sums_ref(g, cpos, S, scale, shift, k):
    """ fp64: dS[n, cls, c] = scale * sum over the pixels of class cls of g * [(cpos + S[cls]) * scale + shift > 0] """
    n, H, W, C = g.shape
    r = k // 2

    def cls_of(p, m):
        return p if p < r else (k - 1 - (m - 1 - p) if p >= m - r else r)
    cy = torch.tensor([cls_of(y, H) for y in range(H)])
    cx = torch.tensor([cls_of(x, W) for x in range(W)])
    cls = (cy[:, None] * k + cx[None, :]).reshape(-1)                           # (H W)
    sc = scale.double() if scale is not None else torch.ones(C, dtype=torch.float64)
    pre = (cpos.double().reshape(1, H * W, C) + S.double()[:, cls]) * sc + shift.double()
    gg = torch.where(pre > 0, g.double().reshape(n, H * W, C), torch.zeros(()).double())
    out = torch.zeros((n, k * k, C), dtype=torch.float64)
    out.index_add_(1, cls, gg)
    return out * sc


@pytest.mark.parametrize("k", [3, 5, 7])
@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("bn", [False, True])
def test_class_reduce_k_matches_fp64_and_expand_adjoint(k, C, bn):
    n, H, W = 3, 8, 11
    gen = torch.Generator().manual_seed(k * 10 + C + bn)
    g = torch.randn((n, H, W, C), generator=gen) * 1e-7
    cpos = torch.randn((H, W, C), generator=gen)
    S = torch.randn((n, k * k, C), generator=gen)
    scale = (0.5 + torch.rand(C, generator=gen)) if bn else None
    shift = torch.randn(C, generator=gen) * 0.3
    dev = [t.to(DEV) if t is not None else None for t in (g, cpos, S, scale, shift)]
    dS = K.dec_class_reduce_k(*dev, k)
    dS2 = K.dec_class_reduce_k(*dev, k)
    torch.cuda.synchronize()
    ref = _class_sums_ref(g, cpos, S, scale, shift, k)
    err = (dS.double().cpu() - ref).abs().max().item() / ref.abs().max().item()
    assert err < 1e-5, err
    assert torch.equal(dS, dS2)
    # adjoint identity with the forward: <g, d expand(S; dir)> = <dS, dir>, d expand = gate * scale * dir[cls]
    dirn = torch.randn((n, k * k, C), generator=gen).to(DEV)
    y = K.dec_layer0_expand(dev[1], dev[2], dev[3], dev[4], k, relu=True)
    lin = K.dec_layer0_expand(torch.zeros_like(dev[1]), dirn, dev[3], torch.zeros_like(dev[4]), k, relu=False)
    lhs = (dev[0].double() * (y > 0).double() * lin.double()).sum().item()
    rhs = (dS.double() * dirn.double()).sum().item()
    assert abs(lhs - rhs) <= 1e-5 * (dev[0].double().abs() * lin.double().abs()).sum().item()


# ---- GenericDecoderLoss against autograd ----------------------------------------------------------------------------
def manifest(tag):
    with open(os.path.join(GOLDEN, f"state_dict_manifest_savi_{tag}.json")) as f:
        return json.load(f)


def build(tag, Ks=7, num_preds=2):
    model_params = copy.deepcopy(manifest(tag)["model_params"])
    model_params["num_slots"] = Ks
    exp = default_exp_params(num_slots=Ks, num_context=1, num_preds=num_preds)
    exp["model"]["model_params"] = model_params
    savi = setup_model(exp["model"]).eval()
    pred = setup_predictor(exp).eval()
    synth.fill_module_(savi, prefix="savi.")
    synth.fill_batchnorm_stats_(savi, prefix="savi.")
    synth.fill_module_(pred, prefix="pred.")
    return savi.to(DEV), pred.to(DEV)


def ref_decode(savi, slots, gates=None, masks=None):
    """ reference-form SAVi decode in fp64 on the CPU (broadcast + position table, [conv, eval BN, ReLU, x2 nearest] per
    block, 3x3 tail, softmax over the slots, compositing) -> (F, 3, H, W).  ``gates`` / ``masks`` (gpu_forward): every
    ReLU is replaced by its 0/1 pattern on the GPU's forward and the slot masks are the GPU's, so that the reference is the
    exact derivative of the function the kernels differentiate at the point where they differentiate it (a pre-activation
    within fp32 rounding of zero takes either side of the ReLU; a mask of e^-30 carries the logit's absolute fp32 error as
    its relative error -- test_decoder_backward_gpu.py::oracle_loss_grad) """
    dec = savi.decoder
    F_, Ks, D = slots.shape
    pos = savi.decoder_pos_embedding.table().detach().double().cpu()                # (H0, W0, D)
    x = slots.reshape(F_ * Ks, D, 1, 1) + pos.permute(2, 0, 1)[None]
    L = len(dec.hidden_dims)
    for j in range(L):
        blk = dec.decoder[dec._block_idx[j]]
        cw = blk.conv
        x = F.conv2d(x, cw.weight.detach().double().cpu(), cw.bias.detach().double().cpu(), padding=dec.kernel_size // 2)
        if dec.batch_norm:
            bn = blk.block[1]
            x = F.batch_norm(x, bn.running_mean.double().cpu(), bn.running_var.double().cpu(),
                             bn.weight.detach().double().cpu(), bn.bias.detach().double().cpu(), False, 0.0, bn.eps)
        x = F.relu(x) if gates is None else x * gates[j]
        if dec.upsample and j < L - 1:
            x = F.interpolate(x, scale_factor=2, mode="nearest")
    tail = dec.decoder[dec._tail_idx]
    y = F.conv2d(x, tail.weight.detach().double().cpu(), tail.bias.detach().double().cpu(), padding=1)
    y = y.reshape(F_, Ks, 4, *y.shape[-2:])
    alpha = y[:, :, 3:]
    m = torch.softmax(alpha, dim=1) if masks is None else torch.softmax(masks.double().log() + (alpha - alpha.detach()), 1)
    return (y[:, :, :3] * m).sum(dim=1)


@torch.no_grad()
def gpu_forward(savi, slots):
    """ (the ReLU patterns (NCHW 0/1 fp64 on the CPU) of every hidden block, the slot masks) of the forward that
    GenericDecoderLoss runs (the calls of ConvDecoder._decode_generic) """
    dec = savi.decoder
    F_, Ks, D = slots.shape
    k, prec = dec.kernel_size, dec.generic_precision
    cpos, tapsum = dec._generic_layer0(savi.decoder_pos_embedding.table())
    n = F_ * Ks
    S = K.linear(slots.reshape(n, D), tapsum).reshape(n, k * k, cpos.shape[-1])
    acts = [K.dec_layer0_expand(cpos, S, *dec._scale_shift(0), k, relu=True)]
    for j in range(1, len(dec.hidden_dims)):
        acts.append(K.convk(acts[-1], dec._generic_weights(j, prec), *dec._scale_shift(j), k, relu=True,
                            upsample2=bool(dec.upsample), precision=prec))
    tail = dec.decoder[dec._tail_idx]
    masks = K.dec_tail(acts[-1], tail.weight, tail.bias, F_, Ks)[2]
    return [(a > 0).permute(0, 3, 1, 2).double().cpu() for a in acts], masks.cpu()


def ref_loss_grad(savi, slots, targets, grad_scale, fwd=(None, None)):
    s = slots.detach().double().cpu().requires_grad_(True)
    img = ref_decode(savi, s, *fwd)
    sq = ((img - targets.double().cpu()) ** 2).sum()
    (ds,) = torch.autograd.grad(sq * (grad_scale / 2), s)
    return sq.item(), ds


def _inputs(savi, F_, Ks, seed):
    H, W = savi.decoder.output_size(tuple(savi.decoder_pos_embedding.resolution))
    gen = torch.Generator().manual_seed(seed)
    slots = torch.randn((F_, Ks, 128), generator=gen)
    targets = torch.rand((F_, 3, H, W), generator=gen)
    return slots.to(DEV), targets.to(DEV)


def _check_against_ref(savi, slots, targets, grad_scale, fpc=None):
    from textocvp_amd.train.decoder_generic import GenericDecoderLoss
    loss = GenericDecoderLoss(savi, frames_per_chunk=fpc)
    sq, ds = loss.loss_and_slot_grad(slots, targets, grad_scale)
    torch.cuda.synchronize()
    sq_ref, ds_ref = ref_loss_grad(savi, slots, targets, grad_scale, gpu_forward(savi, slots))
    assert abs(sq.item() - sq_ref) <= 1e-5 * sq_ref, (sq.item(), sq_ref)
    d = (ds.double().cpu() - ds_ref).abs()
    for f in range(ds.shape[0]):
        bar = 2e-4 * ds_ref[f].abs().max().item()
        assert d[f].max().item() <= bar, (f, d[f].max().item(), bar)
    return sq, ds


# (tag, slots, frames): K = 7 on every variant, K = 30 where the fp64 reference stays affordable
CASES = [("up2", 7, 3), ("k3", 7, 3), ("bn_up2_128", 7, 1), ("k7_mixed", 7, 2), ("up2", 30, 2), ("k3", 30, 1)]


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
@pytest.mark.parametrize("tag,Ks,F_", CASES)
def test_generic_decoder_loss_against_autograd(tag, Ks, F_, precision, monkeypatch):
    savi, _ = build(tag, Ks=Ks)
    savi.decoder.generic_precision = precision
    slots, targets = _inputs(savi, F_, Ks, seed=Ks + F_)
    grad_scale = 2.0 / targets.numel()
    # the forward images are those of SAVi.decode, bit for bit
    seen = []
    orig = K.dec_tail

    def recording(*a, **kw):
        out = orig(*a, **kw)
        seen.append(out[0].clone())
        return out
    monkeypatch.setattr(K, "dec_tail", recording)
    sq, ds = _check_against_ref(savi, slots, targets, grad_scale)
    monkeypatch.undo()
    with torch.no_grad():
        imgs = savi.decode(slots)["recons_imgs"]
    assert torch.equal(seen[0], imgs)                           # one chunk; seen[1] is gpu_forward's
    # chunked one frame at a time and at max_slot_images: the same bits
    from textocvp_amd.train.decoder_generic import GenericDecoderLoss
    sq1, ds1 = GenericDecoderLoss(savi, frames_per_chunk=1).loss_and_slot_grad(slots, targets, grad_scale)
    assert torch.equal(ds1, ds) and abs(sq1.item() - sq.item()) <= 1e-6 * sq.item()
    savi.decoder.max_slot_images = Ks
    sq2, ds2 = GenericDecoderLoss(savi).loss_and_slot_grad(slots, targets, grad_scale)
    assert torch.equal(ds2, ds)


def test_generic_decoder_loss_scales_and_non_finite_targets():
    from textocvp_amd.train.decoder_generic import GenericDecoderLoss
    savi, _ = build("up2")
    slots, targets = _inputs(savi, 2, 7, seed=5)
    loss = GenericDecoderLoss(savi)
    sq, ds = loss.loss_and_slot_grad(slots, targets, 1e-6)
    sq0, ds0 = loss.loss_and_slot_grad(slots, targets, 0.0)
    assert torch.equal(sq0, sq) and (ds0 == 0).all()
    sq4, ds4 = loss.loss_and_slot_grad(slots, targets, 4e-6)
    assert torch.equal(ds4, ds * 4)
    sqs, dss = loss.loss_and_slot_grad(slots, targets, 1e-6 * 2.0 ** -20)
    assert torch.equal(dss, ds * 2.0 ** -20)
    bad = targets.clone()
    bad[1, 0, 3, 5] = float("nan")
    sqn, dsn = loss.loss_and_slot_grad(slots, bad, 1e-6)
    assert not torch.isfinite(sqn).all() and not torch.isfinite(dsn[1]).all()
    assert torch.equal(dsn[0], ds[0])
    with pytest.raises(ValueError):
        loss.loss_and_slot_grad(slots, targets[..., :32, :32].contiguous(), 1e-6)


def test_generic_decoder_loss_follows_weight_and_statistic_changes():
    from textocvp_amd.train.decoder_generic import GenericDecoderLoss
    savi, _ = build("bn_up2_128")
    slots, targets = _inputs(savi, 1, 7, seed=9)
    loss = GenericDecoderLoss(savi)
    _, ds1 = loss.loss_and_slot_grad(slots, targets, 1e-6)
    dec = savi.decoder
    with torch.no_grad():
        dec.decoder[dec._block_idx[2]].conv.weight.mul_(1.25)
        dec.decoder[dec._block_idx[3]].block[1].running_var.mul_(0.5)
    _, ds2 = loss.loss_and_slot_grad(slots, targets, 1e-6)
    _, ds3 = GenericDecoderLoss(copy.deepcopy(savi)).loss_and_slot_grad(slots, targets, 1e-6)
    assert not torch.equal(ds1, ds2)
    assert torch.equal(ds2, ds3)
    _check_against_ref(savi, slots, targets, 1e-6)


def test_generic_decoder_loss_graph_replay_is_bit_identical():
    from textocvp_amd.train.decoder_generic import GenericDecoderLoss
    savi, _ = build("up2")
    slots, targets = _inputs(savi, 2, 7, seed=3)
    loss = GenericDecoderLoss(savi)
    sq, ds = loss.loss_and_slot_grad(slots, targets, 1e-6)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = loss.loss_and_slot_grad(slots, targets, 1e-6)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0], sq) and torch.equal(out[1], ds)


# ---- the whole training step ----------------------------------------------------------------------------------------
def _step(tag, **kw):
    from textocvp_amd.train.step import PredictorTrainStep
    savi, pred = build(tag)
    ts = PredictorTrainStep(savi, pred, lr=1e-4, clip=0.05, warmup_steps=0, text_dropout=0.0, **kw)
    H, W = savi.decoder.output_size(tuple(savi.decoder_pos_embedding.resolution))
    videos = synth.synth_videos(2, 3, height=H, width=W, seed=0).to(DEV)
    tokens, lengths = synth.synth_captions(2, max_len=10, seed=0)
    noise = synth.synth_noise(2, 7, 128, seed=1).to(DEV)
    return ts, (videos, tokens.to(DEV), lengths.to(DEV)), noise


@pytest.mark.parametrize("tag", VARIANTS)
def test_training_step_runs_on_variant(tag):
    from textocvp_amd.train.decoder_generic import GenericDecoderLoss
    ts, args, noise = _step(tag)
    assert isinstance(ts.decoder, GenericDecoderLoss)
    res = ts.step(*args, init_noise=noise)
    assert all(np.isfinite(res[k]) for k in ("loss", "pred_img_mse", "pred_slot_mse", "grad_norm"))
    assert res["pred_img_mse"] > 0 and res["grad_norm"] > 0


def test_graph_replayed_steps_match_eager_steps_on_up2():
    res = []
    for graphed in (False, True):
        ts, args, noise = _step("up2")
        run = ts.step_graphed if graphed else ts.step
        res.append([dict(run(*args, init_noise=noise)) for _ in range(3)])
    for a, b in zip(*res):
        assert abs(a["loss"] - b["loss"]) < 1e-5 * abs(a["loss"])
        assert abs(a["grad_norm"] - b["grad_norm"]) < 1e-4 * a["grad_norm"]
    assert res[0][0]["loss"] != res[0][2]["loss"]


def test_forced_range_fallback_on_variant_ends_on_fp32(monkeypatch):
    ts_ref, args, noise = _step("up2")
    ts_ref.savi.decoder.generic_precision = "fp32"
    ref = ts_ref.loss_and_grads(*args, init_noise=noise)
    gref = {n: v.grad.clone() for n, v in ts_ref.model.names.items()}
    ts, args, noise = _step("up2")
    if ts.savi.decoder.generic_precision != "f16x3":
        pytest.skip("arithmetic already fp32 (TOCVP_PRECISION=fp32)")
    real = K._check_f16_range

    def decoder_only(amax, what, owner=None):                 # only the decoder's convk operands count as saturated
        return real(float("inf") if what.startswith("convk") else amax, what, owner)
    monkeypatch.setattr(K, "_check_f16_range", decoder_only)
    with pytest.warns(UserWarning, match="fp32-range fallback"):
        got = ts.loss_and_grads(*args, init_noise=noise)
    assert ts.savi.decoder.generic_precision == "fp32"
    assert abs(got["pred_img_mse"] - ref["pred_img_mse"]) <= 1e-6 * ref["pred_img_mse"]
    for n, v in ts.model.names.items():
        d = (v.grad - gref[n]).abs().max().item()
        assert d <= 2e-4 * max(gref[n].abs().max().item(), 1e-30), n


@pytest.mark.parametrize("tag", VARIANTS)
def test_training_step_against_reference_golden(tag):
    """ losses and gradient norms of the reference's own training step on the frozen variant (train_savi_<tag>.npz,
    tests/golden/make_golden_train_savi_variants.py); the bars of
    test_train_dinosaur_gpu.py::test_training_step_against_reference_golden """
    from conftest import load_golden
    g = load_golden(f"train_savi_{tag}.npz")
    ts, _, _ = _step(tag)
    H, W = ts.savi.decoder.output_size(tuple(ts.savi.decoder_pos_embedding.resolution))
    videos = synth.synth_videos(2, 3, height=H, width=W, seed=0).to(DEV)
    noise = synth.synth_noise(2, 7, 128, seed=1).to(DEV)
    tokens, lengths = torch.from_numpy(g["tokens"]).to(DEV), torch.from_numpy(g["lengths"]).to(DEV)
    losses = ts.loss_and_grads(videos, tokens, lengths, init_noise=noise)
    e_img = abs(losses["pred_img_mse"] - float(g["loss_img"])) / float(g["loss_img"])
    e_slot = abs(losses["pred_slot_mse"] - float(g["loss_slot"])) / float(g["loss_slot"])
    assert e_img < 2e-4 and e_slot < 2e-4, (e_img, e_slot)
    worst = 0.0
    for name, ref_norm in zip(g["names"], g["grad_norms"]):
        v = ts.model.names.get(str(name))
        if v is None:
            assert float(ref_norm) == 0.0, str(name)
            continue
        norm = 0.0 if v.grad is None else float(v.grad.norm())
        e = abs(norm - float(ref_norm)) / max(float(ref_norm), 1e-8)
        worst = max(worst, e if float(ref_norm) > 1e-7 else 0.0)
        assert e < 5e-3 or abs(norm - float(ref_norm)) < 1e-8, (str(name), norm, float(ref_norm))
    for key in g:
        if key.startswith("grad::"):
            grad = ts.model.names[key[6:]].grad
            if grad.dim() == 2 and grad.numel() > 40000:
                grad = grad[::4, ::4]
            ref = torch.from_numpy(g[key]).double()
            err = (grad.reshape(ref.shape).detach().cpu().double() - ref).abs().max().item() / ref.abs().max().item()
            assert err < 5e-3, (key, err)
    print(f"[train-savi-{tag}] vs reference golden: losses {e_img:.1e} / {e_slot:.1e}, worst gradient norm {worst:.2e}")
