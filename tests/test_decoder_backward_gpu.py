"""
The image-loss backward through the frozen SAVi decoder (train/decoder.py, DecoderLoss.loss_and_slot_grad) against
float64 references: each of its kernels alone (tocvp_mse_f32, tocvp_dec_tail_grad_f32, tocvp_conv3x3_t4_f32,
tocvp_dec_class_reduce_f32) at shapes that run their grid-stride loops and edge cases, then the whole backward against
torch.autograd on the oracle decoder in float64 -- every arithmetic of the decoder convs, chunked and unchunked,
synth and saturated masks, zero / tiny / huge loss scales, non-finite targets and decoder weights that change after
the first call.  Needs a real MI355X (pytest -m gpu).
"""

import copy
import functools
import hashlib

import pytest
import torch
import torch.nn.functional as F

from textocvp_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
D = 128                     # slot dimension of the reference SAVi config
RES = (64, 64)


def _L():
    from textocvp_amd import kernels as K
    return K.lib()


def _s():
    return torch.cuda.current_stream().cuda_stream


def rnd(name, shape, dist="normal", scale=1.0, seed=0):
    return synth.synth_tensor("decbwd." + name, shape, dist, scale, seed)


# ---------------------------------------------------------------------------------------------------------------
# kernels one by one

@pytest.mark.parametrize("n", [1, 255, 3 * 64 * 64 * 23 + 5])
@pytest.mark.parametrize("nblocks", [1, 7, 1024])
@pytest.mark.parametrize("with_dpred", [False, True])
def test_mse_partials_and_gradient(n, nblocks, with_dpred):
    """ sum of the block partials = sum (p - t)^2 in fp64; dpred = gscale * (p - t) rounded once, as torch has it """
    p = rnd("mse.p", (n,)).to(DEV)
    t = rnd("mse.t", (n,), "uniform").to(DEV)
    gscale = 0.37
    part = torch.full((nblocks,), float("nan"), device=DEV)
    dpred = torch.full((n,), float("nan"), device=DEV) if with_dpred else None
    rc = _L().tocvp_mse_f32(p.data_ptr(), t.data_ptr(), part.data_ptr(), nblocks,
                            dpred.data_ptr() if with_dpred else None, n, gscale, _s())
    assert rc == 0
    torch.cuda.synchronize()
    ref = ((p.double() - t.double()) ** 2).sum().item()
    got = part.double().sum().item()
    assert abs(got - ref) <= 1e-6 * ref, (got, ref)
    if with_dpred:
        assert torch.equal(dpred, gscale * (p - t))


@pytest.mark.parametrize("F_", [1, 3])
@pytest.mark.parametrize("Kn", [1, 7, 30])
@pytest.mark.parametrize("HW", [(64, 64), (5, 12)])
def test_dec_tail_grad(F_, Kn, HW):
    """ dy (F*K, H, W, 4) = [d rgb_k | d alpha_k] of img = sum_k rgb_k * softmax_k(alpha), logits spread to +-40 so
    that some masks are exactly 0 or 1 in fp32 """
    H, W = HW
    alpha = rnd("tail.alpha", (F_, Kn, 1, H, W), "uniform", 40.0).double()
    alpha[:, 0, :, ::2, :] = 120.0                      # every other row: a logit gap > 104, m = 1 and 0 exactly in fp32
    alpha.requires_grad_(True)
    rgb = rnd("tail.rgb", (F_, Kn, 3, H, W)).double().requires_grad_(True)
    dimg = rnd("tail.dimg", (F_, 3, H, W)).double()
    masks = torch.softmax(alpha, dim=1)
    (rgb.float().double() * masks).sum(1).backward(dimg)
    ref = torch.cat([rgb.grad.permute(0, 1, 3, 4, 2), alpha.grad.permute(0, 1, 3, 4, 2)], -1).reshape(F_ * Kn, H, W, 4)

    m32 = masks.detach().float().contiguous()
    if Kn > 1:
        assert (m32 == 0).any() and (m32 == 1).any()
    rgb32, dimg32 = rgb.detach().float().contiguous().to(DEV), dimg.float().contiguous().to(DEV)
    dy = torch.full((F_ * Kn, H, W, 4), float("nan"), device=DEV)
    assert _L().tocvp_dec_tail_grad_f32(dimg32.data_ptr(), rgb32.data_ptr(), m32.to(DEV).data_ptr(), dy.data_ptr(),
                                        F_, Kn, H, W, _s()) == 0
    got = dy.cpu().double()
    for sl, what in ((slice(0, 3), "rgb"), (slice(3, 4), "alpha")):
        r, g = ref[..., sl], got[..., sl]
        if what == "alpha" and Kn == 1:
            assert torch.equal(got[..., 3], torch.zeros_like(got[..., 3]))        # softmax over one slot: m = 1
            continue
        err = (g - r).abs().max().item()
        assert err <= 1e-6 * r.abs().max().item(), (what, err, r.abs().max().item())


def _conv3x3_t4_ref(dy, w, act):
    """ autograd of conv2d(x, w, padding=1) (C -> 4) w.r.t. x, times relu'(act) (relu'(0) = 0) -- NHWC """
    n, H, W, C = act.shape
    x = torch.zeros(n, C, H, W, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, w.double(), padding=1).backward(dy.double().permute(0, 3, 1, 2))
    return x.grad.permute(0, 2, 3, 1) * (act.double() > 0)


@pytest.mark.parametrize("n,H,W,C", [(3, 64, 64, 64), (70, 64, 64, 64), (2, 7, 12, 4), (2, 7, 12, 32),
                                     (2, 6, 8, 4), (2, 6, 8, 32)])
def test_conv3x3_t4(n, H, W, C):
    """ transposed 3x3 tail conv (4 -> C) fused with the ReLU mask; n = 70 slot images of 64x64 run the grid-stride
    loop past its first pass (4096 workgroups cover 65) """
    dy = rnd("t4.dy", (n, H, W, 4))
    w = rnd("t4.w", (4, C, 3, 3), "normal", 0.2)
    act = rnd("t4.act", (n, H, W, C))
    act[rnd("t4.zero", (n, H, W, C), "unit") < 0.2] = 0.0                       # exact zeros: gate off
    assert (act == 0).any() and (act < 0).any()
    ref = _conv3x3_t4_ref(dy, w, act)
    dx = torch.full((n, H, W, C), float("nan"), device=DEV)
    dyd, wd, actd = dy.to(DEV), w.to(DEV), act.to(DEV)
    assert _L().tocvp_conv3x3_t4_f32(dyd.data_ptr(), wd.data_ptr(), actd.data_ptr(), dx.data_ptr(), n, H, W, C,
                                     _s()) == 0
    got = dx.cpu().double()
    assert torch.equal(got[act <= 0], torch.zeros_like(got[act <= 0]))
    err = (got - ref).abs().max().item()
    assert err <= 1e-6 * ref.abs().max().item(), (err, ref.abs().max().item())


@pytest.mark.parametrize("case", ["w_not_4", "c_over_64", "c_not_4", "misaligned"])
def test_conv3x3_t4_rejects_bad_arguments(case):
    """ every refused call returns an error code and leaves the output untouched (buffers sized for the claimed
    shape, so nothing would be out of bounds even if a check were missing) """
    n, H, W, C = 2, 8, 8, 32
    if case == "w_not_4":
        W = 10
    elif case == "c_over_64":
        C = 68
    elif case == "c_not_4":
        C = 30
    dy = torch.ones(n * H * W * 4 + 4, device=DEV)
    w = torch.ones(4 * C * 9, device=DEV)
    act = torch.ones(n * H * W * C + 4, device=DEV)
    dx = torch.full((n * H * W * C + 4,), 7.0, device=DEV)
    off = 4 if case == "misaligned" else 0                                           # 4 bytes: not 16-aligned
    rc = _L().tocvp_conv3x3_t4_f32(dy.data_ptr() + off, w.data_ptr(), act.data_ptr(), dx.data_ptr() + off,
                                   n, H, W, C, _s())
    torch.cuda.synchronize()
    assert rc != 0, case
    assert torch.equal(dx, torch.full_like(dx, 7.0)), case


def _border_cls(p, n):
    return p if p < 2 else (4 - (n - 1 - p) if p >= n - 2 else 2)


@pytest.mark.parametrize("n", [1, 37])
@pytest.mark.parametrize("HW", [(64, 64), (4, 4), (5, 9), (8, 64)])
def test_dec_class_reduce(n, HW):
    """ dS[n, cls, c] = sum over the pixels of border class cls of g * (cpos + S[cls] > 0), with cpos + S == 0
    exactly at some entries (gate off); bound relative to the class's sum of |g| (LDS atomics: any order) """
    H, W = HW
    C = 64
    g = rnd("cr.g", (n, H, W, C))
    cpos = rnd("cr.cpos", (H, W, C))
    S = rnd("cr.S", (n, 25, C), "normal", 0.5)
    cls = torch.tensor([[_border_cls(y, H) * 5 + _border_cls(x, W) for x in range(W)] for y in range(H)])
    # image 0: cpos = -S exactly on a fifth of the (pixel, channel) entries
    hit = rnd("cr.hit", (H, W, C), "unit") < 0.2
    s0 = S[0][cls]                                                                 # (H, W, C)
    cpos[hit] = -s0[hit]
    assert ((cpos + S[0][cls]) == 0).sum().item() >= hit.sum().item()
    gate = (cpos[None].double() + S.double()[:, cls]) > 0                          # (n, H, W, C)
    onehot = F.one_hot(cls.reshape(-1), 25).double()                               # (HW, 25)
    gg = (g.double() * gate).reshape(n, H * W, C)
    ref = torch.einsum("pk,npc->nkc", onehot, gg)
    bound = torch.einsum("pk,npc->nkc", onehot, g.double().abs().reshape(n, H * W, C))
    dS = torch.full((n, 25, C), float("nan"), device=DEV)
    gd, cd, Sd = g.to(DEV), cpos.contiguous().to(DEV), S.to(DEV)
    assert _L().tocvp_dec_class_reduce_f32(gd.data_ptr(), cd.data_ptr(), Sd.data_ptr(), dS.data_ptr(), n, H, W, C,
                                           _s()) == 0
    got = dS.cpu().double()
    empty = bound == 0                                                             # classes without pixels
    assert torch.equal(got[empty], torch.zeros_like(got[empty]))
    assert ((got - ref).abs() <= 1e-6 * bound).all(), ((got - ref).abs() / bound.clamp_min(1e-30)).max().item()


# ---------------------------------------------------------------------------------------------------------------
# the whole DecoderLoss.loss_and_slot_grad against torch.autograd on the fp64 oracle decoder

@functools.lru_cache(maxsize=None)
def _savi_cpu(saturated, seed=0):
    from textocvp_amd.setup_model import default_exp_params, setup_model
    savi = setup_model(default_exp_params(num_slots=7, num_context=1, num_preds=2)["model"]).eval()
    synth.fill_module_(savi, seed=seed, prefix="savi.")
    if saturated:
        # the alpha row of the tail conv x 30: near one-hot masks as in a trained decoder
        tail = savi.decoder.decoder[len(savi.decoder.hidden_dims)]
        with torch.no_grad():
            tail.weight[3].mul_(30.0)
    return savi


def _savi(saturated=False):
    return copy.deepcopy(_savi_cpu(saturated)).to(DEV)


def _inputs(Ks, F_):
    slots = rnd("e2e.slots", (F_, Ks, D), seed=Ks)
    targets = rnd("e2e.targets", (F_, 3) + RES, "unit", seed=Ks)
    return slots, targets


def _gscale(targets):
    return 2.0 / targets.numel()                                                   # 1.0 * MSE


def oracle_loss_grad(sd, slots, targets, grad_scale, gates=None, masks=None):
    """ (sum (img - target)^2, d/d slots of grad_scale / 2 * sum (img - target)^2), all in float64.

    gates, masks (optional, from ``gpu_forward``): the ReLU of every hidden conv layer is replaced by its 0/1 pattern
    on the GPU's forward, and the slot masks are the GPU's.  The loss is piecewise smooth in the slots: where a pre-activation lies within fp32 rounding of
    zero, the fp32 and fp64 forwards can take different sides of the ReLU, and the two gradients then differ by that
    unit's whole contribution -- even plain fp32 torch.autograd on the CPU is 1e-4 .. 1e-3 (of the frame maximum) away
    from fp64 autograd on these decoders.  With the GPU's gates the reference is the exact derivative of the function
    the kernels differentiate at the point where they differentiate it, and the comparison measures the backward's
    arithmetic alone (the forward has parity tests of its own).  """
    from oracle import slot_rollout_oracle as O
    sd64 = {k: (v.detach().cpu().double() if v.is_floating_point() else v.cpu()) for k, v in sd.items()}
    s = slots.double().clone().requires_grad_(True)
    if gates is None:
        img, _, _ = O.savi_decode(sd64, s, RES, 3)
    else:
        Fn, Kn, _ = s.shape
        pos = O.soft_pos_embed(sd64["decoder_pos_embedding.projection.weight"],
                               sd64["decoder_pos_embedding.projection.bias"], RES)
        x = (s.reshape(Fn * Kn, 1, 1, D) + pos[None]).permute(0, 3, 1, 2)
        for i, gate in enumerate(gates):
            w, b = sd64[f"decoder.decoder.{i}.block.0.weight"], sd64[f"decoder.decoder.{i}.block.0.bias"]
            x = F.conv2d(x, w, b, padding=2) * gate
        y = F.conv2d(x, sd64["decoder.decoder.4.weight"], sd64["decoder.decoder.4.bias"], padding=1)
        y = y.reshape(Fn, Kn, 4, *RES)
        alpha = y[:, :, 3:]
        # the masks of the GPU forward (softmax Jacobian taken there): a mask of e^-30 carries the logit's ABSOLUTE
        # fp32 error as its relative error, which would otherwise dominate the gradient of a slot made of such pixels
        m = torch.softmax(masks.double().log() + (alpha - alpha.detach()), dim=1)
        img = (y[:, :, :3] * m).sum(1)
    d = img - targets.double()
    sq = (d * d).sum()
    (grad_scale / 2 * sq).backward()
    return sq.item(), s.grad


@torch.no_grad()
def gpu_forward(savi, slots, fpc):
    """ (the ReLU patterns (x > 0, as NCHW bool on the CPU) of the four hidden layers, the slot masks (F, K, 1, H, W))
    of the GPU forward that DecoderLoss.loss_and_slot_grad runs on ``slots`` with ``fpc`` frames per chunk, under the
    current arithmetic """
    from textocvp_amd import kernels as K
    from textocvp_amd.train.decoder import DecoderLoss
    loss, dec = DecoderLoss(savi), savi.decoder
    H, W = RES
    cpos, tapsum = dec._collapsed_layer0(savi.decoder_pos_embedding.table())
    cls = torch.tensor([[_border_cls(y, H) * 5 + _border_cls(x, W) for x in range(W)] for y in range(H)],
                       device=DEV)
    out, masks = [[] for _ in range(4)], []
    Fn, Kn, _ = slots.shape
    for f0 in range(0, Fn, fpc):
        n = (min(Fn, f0 + fpc) - f0) * Kn
        S = K.linear(slots[f0:f0 + fpc].reshape(n, D).contiguous().to(DEV), tapsum).reshape(n, 25, 64)
        x1 = loss._conv_fwd(1, None, collapsed=(cpos, S))
        x2 = loss._conv_fwd(2, x1)
        x3 = loss._conv_fwd(3, x2)
        for li, act in enumerate((cpos[None] + S[:, cls], x1, x2, x3)):
            out[li].append((act > 0).permute(0, 3, 1, 2).cpu())
        tail = dec.decoder[4]
        masks.append(K.dec_tail(x3, tail.weight, tail.bias, n // Kn, Kn)[2].cpu())
    return [torch.cat(o) for o in out], torch.cat(masks)


@pytest.fixture(scope="module")
def reference():
    """ fp64 references, computed once per (shape, synth / saturated, GPU forward state) and shared by every arithmetic and
    chunking that has that pattern """
    cache = {}

    def get(Ks, F_, saturated, fwd):
        gates, masks = fwd
        key = (Ks, F_, saturated, hashlib.sha1(b"".join(t.numpy().tobytes() for t in gates + [masks])).hexdigest())
        if key not in cache:
            slots, targets = _inputs(Ks, F_)
            cache[key] = oracle_loss_grad(_savi_cpu(saturated).state_dict(), slots, targets, _gscale(targets), *fwd)
        return cache[key]
    return get


# arithmetic of the decoder convs: (conv_precision, conv_wino, Winograd data gradient) and the frame bound
ARITH = {
    "wino": ("f16x3", True, True, 3e-5),            # default: Winograd forward and data gradient
    "wino_fwd_bf16x3_dgrad": ("f16x3", True, False, 3e-5),
    "f16x3": ("f16x3", False, True, 3e-5),          # direct f16x3 forward (its data gradient runs on bf16x3)
    "bf16x3": ("bf16x3", False, True, 2e-4),
}
BINS = ((2.0 ** -12, ">= 2^-12"), (2.0 ** -20, "2^-12..2^-20"), (2.0 ** -30, "2^-20..2^-30"), (0.0, "< 2^-30"))


def _image_tol(Ks, saturated, arith):
    """ bound of one slot image's error relative to its own max |ref|, for images >= 2^-12 of their chunk's maximum.
    1e-4 everywhere but one image of the Ks = 30 saturated set (2^-10.5 of its chunk): measured 1.1e-4 under the
    Winograd forward with either data gradient (Winograd or bf16x3 -- so not the Winograd per-chunk operand scale),
    6.7e-5 under the direct f16x3 forward and 3.2e-4 under the bf16x3 forward: it follows the forward arithmetic, not
    the backward's. """
    if saturated and Ks == 30:
        return 5e-4 if ARITH[arith][0] == "bf16x3" else 2e-4
    return 1e-4


def _set_arith(savi, arith, monkeypatch):
    from textocvp_amd.train import decoder as dmod
    prec, wino, wdg, tol = ARITH[arith]
    savi.decoder.conv_precision, savi.decoder.conv_wino = prec, wino
    monkeypatch.setattr(dmod, "_WINO_DGRAD", wdg)
    return tol


def _default_tol(savi):
    """ bound of the default arithmetic: TOCVP_PRECISION=fp32 leaves DecoderLoss on bf16x3 """
    return 3e-5 if savi.decoder.conv_precision == "f16x3" else 2e-4


def _frame_errors(got, ref):
    """ per frame: max |got - ref| / max |ref| """
    got = got.cpu().double()
    return [((got[f] - ref[f]).abs().max() / ref[f].abs().max()).item() for f in range(ref.shape[0])]


def _per_image(got, ref, fpc):
    """ (ratio of the image's max |ref| to its chunk's, relative error of the image) for every slot image """
    got = got.cpu().double()
    out = []
    for f0 in range(0, ref.shape[0], fpc):
        ch = ref[f0:f0 + fpc]
        cmax = ch.abs().max().item()
        for f in range(f0, min(ref.shape[0], f0 + fpc)):
            for k in range(ref.shape[1]):
                m = ref[f, k].abs().max().item()
                out.append((m / cmax, (got[f, k] - ref[f, k]).abs().max().item() / max(m, 1e-300)))
    return out


@pytest.mark.parametrize("Ks,F_", [(7, 3), (30, 2)])
@pytest.mark.parametrize("saturated", [False, True], ids=["synth", "saturated"])
@pytest.mark.parametrize("arith", list(ARITH))
@pytest.mark.parametrize("chunking", ["whole", "fpc1", "fpc2", "max_slot_images"])
def test_loss_and_slot_grad_matches_fp64_autograd(Ks, F_, saturated, arith, chunking, reference, monkeypatch):
    from textocvp_amd.train.decoder import DecoderLoss
    savi = _savi(saturated)
    tol = _set_arith(savi, arith, monkeypatch)
    fpc = {"whole": None, "fpc1": 1, "fpc2": 2, "max_slot_images": None}[chunking]
    if chunking == "max_slot_images":
        savi.decoder.max_slot_images = 2 * Ks + 1                                  # 2 frames per chunk
    used = fpc or max(1, savi.decoder.max_slot_images // Ks)
    slots, targets = _inputs(Ks, F_)
    sq_ref, ref = reference(Ks, F_, saturated, gpu_forward(savi, slots, used))
    sq, ds = DecoderLoss(savi, frames_per_chunk=fpc).loss_and_slot_grad(slots.to(DEV), targets.to(DEV),
                                                                        _gscale(targets))
    torch.cuda.synchronize()
    e_sq = abs(sq.item() - sq_ref) / sq_ref
    fe = _frame_errors(ds, ref)
    imgs = _per_image(ds, ref, used)
    worst = {name: max([e for r, e in imgs if lo <= r < (BINS[i - 1][0] if i else float("inf"))], default=None)
             for i, (lo, name) in enumerate(BINS)}
    print(f"\n[dec-bwd] Ks={Ks} F={F_} {'saturated' if saturated else 'synth'} {arith} frames/chunk={used}: "
          f"sq {e_sq:.1e}, frame max {max(fe):.2e} (tol {tol:.0e}); worst per-image by ratio to chunk max: "
          + ", ".join(f"{n} {'-' if w is None else f'{w:.1e}'}" for n, w in worst.items())
          + f"; smallest ratio {min(r for r, _ in imgs):.1e}")
    assert e_sq <= 1e-5, e_sq
    assert max(fe) <= tol, fe
    bad = [(r, e) for r, e in imgs if r >= 2.0 ** -12 and e > _image_tol(Ks, saturated, arith)]
    assert not bad, bad


def _default_run(savi, slots, targets, grad_scale, fpc=None):
    from textocvp_amd.train.decoder import DecoderLoss
    sq, ds = DecoderLoss(savi, frames_per_chunk=fpc).loss_and_slot_grad(slots.to(DEV), targets.to(DEV), grad_scale)
    torch.cuda.synchronize()
    return sq.cpu(), ds.cpu()


EDGE_ARITH = ["default", "bf16x3"]


def _edge_savi(arith, monkeypatch):
    savi = _savi(False)
    if arith != "default":
        _set_arith(savi, arith, monkeypatch)
    return savi


@pytest.mark.parametrize("arith", EDGE_ARITH)
def test_zero_and_power_of_two_grad_scales(arith, monkeypatch):
    """ grad_scale 0: the gradient is exactly zero (the Winograd operand scale of an all-zero input is 2^111, not a
    NaN) and the loss is unchanged; grad_scale 2^-60 / 2^40: the gradient scales by exactly that factor """
    savi = _edge_savi(arith, monkeypatch)
    slots, targets = _inputs(7, 3)
    sq1, ds1 = _default_run(savi, slots, targets, 1.0)
    sq0, ds0 = _default_run(savi, slots, targets, 0.0)
    assert not torch.isnan(ds0).any()
    assert torch.equal(ds0, torch.zeros_like(ds0))
    assert torch.equal(sq0, sq1)
    for e in (-60, 40):
        gs = 2.0 ** e
        _, dsg = _default_run(savi, slots, targets, gs)
        err = (dsg.double() / gs - ds1.double()).abs().max().item()
        assert err <= 1e-6 * ds1.abs().max().item(), (e, err)


@pytest.mark.parametrize("arith", EDGE_ARITH)
@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_non_finite_target_stays_non_finite(arith, bad, monkeypatch):
    """ a NaN / +inf in one target pixel of frame 1 (one frame per chunk): the gradient is non-finite exactly where
    the fp64 reference's is -- nothing non-finite comes out finite -- and frames 0 and 2 are those of a clean run """
    savi = _edge_savi(arith, monkeypatch)
    slots, targets = _inputs(7, 3)
    gs = _gscale(targets)
    _, clean = _default_run(savi, slots, targets, gs, fpc=1)
    tb = targets.clone()
    tb[1, 1, 17, 40] = bad
    _, ds = _default_run(savi, slots, tb, gs, fpc=1)
    _, ref1 = oracle_loss_grad(_savi_cpu(False).state_dict(), slots[1:2], tb[1:2], gs)
    fin = torch.isfinite(ds)
    print(f"\n[dec-bwd] {arith} target {bad}: frame 1 non-finite {int((~fin[1]).sum())} of {fin[1].numel()} "
          f"(reference {int((~torch.isfinite(ref1)).sum())})")
    assert torch.equal(fin[1], torch.isfinite(ref1[0]))
    assert fin[0].all() and fin[2].all()
    for f in (0, 2):
        assert (ds[f] - clean[f]).abs().max().item() <= 1e-6 * clean[f].abs().max().item(), f


@pytest.mark.parametrize("arith", EDGE_ARITH)
@pytest.mark.parametrize("change", ["load_state_dict", "inplace_mul"])
def test_gradient_follows_decoder_weight_changes(arith, change, monkeypatch):
    """ after a first call, the decoder weights change (a second SAVi checkpoint loaded, or one conv weight scaled in
    place under no_grad): the data gradients must use the new weights, as the forward pass does """
    from textocvp_amd.train.decoder import DecoderLoss
    savi = _edge_savi(arith, monkeypatch)
    tol = _default_tol(savi)
    slots, targets = _inputs(7, 3)
    gs = _gscale(targets)
    loss = DecoderLoss(savi)
    loss.loss_and_slot_grad(slots.to(DEV), targets.to(DEV), gs)
    if change == "load_state_dict":
        savi.load_state_dict(_savi_cpu(False, seed=1).state_dict())
    else:
        with torch.no_grad():
            savi.decoder.decoder[2].conv.weight.mul_(-1.5)
    sq, ds = loss.loss_and_slot_grad(slots.to(DEV), targets.to(DEV), gs)
    torch.cuda.synchronize()
    sq_ref, ref = oracle_loss_grad(savi.state_dict(), slots, targets, gs,
                                   *gpu_forward(savi, slots, max(1, savi.decoder.max_slot_images // 7)))
    fe = _frame_errors(ds, ref)
    print(f"\n[dec-bwd] {arith} after {change}: sq {abs(sq.item() - sq_ref) / sq_ref:.1e}, frame max {max(fe):.2e}")
    assert abs(sq.item() - sq_ref) <= 1e-5 * sq_ref
    assert max(fe) <= tol, fe
