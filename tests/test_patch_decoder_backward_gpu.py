"""
The image-loss backward through the frozen ExtendedDINOSAUR decoder (train/patch_decoder.py,
PatchDecoderLoss.loss_and_slot_grad) against float64 references: each new kernel alone (tocvp_conv3x3_dgrad_bf16x3_f32
plain and behind an upsampling, tocvp_bilinear_resize_bwd_f32, tocvp_slot_composite_bwd_f32, tocvp_ln_bcast_bwd_f32)
with adjoint identities, then the whole backward against torch.autograd in float64 on the oracle decoder
(oracle.slot_rollout_oracle.mlp_patch_decoder), chunked and unchunked, two weight families, and the edge cases of the
SAVi decoder tests.  Needs a real MI355X (pytest -m gpu).
"""

from contextlib import contextmanager, nullcontext

import pytest
import torch
import torch.nn.functional as F

from textocvp_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"


def rnd(name, shape, dist="normal", scale=1.0, seed=0):
    return synth.synth_tensor("pdecbwd." + name, shape, dist, scale, seed)


def _rel(got, ref):
    ref = ref.double()
    return (got.detach().cpu().double() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-300)


# ---------------------------------------------------------------------------------------------------------------
# kernels one by one

@pytest.mark.parametrize("up2", [False, True], ids=["plain", "up2"])
@pytest.mark.parametrize("n,H,Cg,Cout", [(1, 16, 64, 128), (2, 24, 32, 64), (3, 5, 96, 192), (1, 9, 32, 768)])
@pytest.mark.parametrize("gated", [False, True])
def test_conv3x3_dgrad_matches_fp64(up2, n, H, Cg, Cout, gated):
    """ dx of y = conv3x3(up2(x) or x) * scale against fp64 autograd; odd sizes leave partial 128-pixel tiles """
    from textocvp_amd import kernels as K
    from textocvp_amd.train.patch_decoder import _dgrad_weights
    W = H + 1 if H % 2 else H
    w = rnd("dg.w", (Cg, Cout, 3, 3), scale=0.1)
    sc = rnd("dg.s", (Cg,), "uniform", 2.0)
    x = rnd("dg.x", (n, Cout, H, W)).double().requires_grad_(True)
    GH, GW = (2 * H, 2 * W) if up2 else (H, W)
    g = rnd("dg.g", (n, Cg, GH, GW), scale=1e-8)                     # the size of an image-loss gradient
    xin = F.interpolate(x, scale_factor=2, mode="nearest") if up2 else x
    F.conv2d(xin, w.double() * sc.double()[:, None, None, None], padding=1).backward(g.double())
    ref = x.grad.permute(0, 2, 3, 1)
    gate = rnd("dg.gate", (n, H, W, Cout)) if gated else None
    if gated:
        ref = ref * (gate.double() > 0)
    got = K.conv3x3_dgrad(g.permute(0, 2, 3, 1).contiguous().to(DEV), _dgrad_weights(w, sc, up2).to(DEV), (H, W),
                          gate=None if gate is None else gate.to(DEV), up2=up2)
    torch.cuda.synchronize()
    err = _rel(got, ref)
    print(f"\n[pdec-bwd] dgrad up2={up2} n={n} {H}x{W} {Cg}->{Cout} gated={gated}: {err:.2e}")
    assert err < 1e-4, err
    if gated:
        assert torch.equal(got.cpu()[gate <= 0], torch.zeros(int((gate <= 0).sum())))


@pytest.mark.parametrize("H", [16, 24, 7])
def test_up2_dgrad_adjoint_identity_fp64(H):
    """ <A x, y> == <x, A^T y> in fp64 for A = nearest x2 -> 3x3 conv: the 16 phase-summed taps of the data
    gradient, applied in fp64 as a stride-2 4x4 correlation, are the exact adjoint of the forward """
    from textocvp_amd.train.patch_decoder import _dgrad_weights
    Cin, Cout = 8, 16
    w = rnd("adj.w", (Cout, Cin, 3, 3)).double()
    x = rnd("adj.x", (2, Cin, H, H)).double()
    y = rnd("adj.y", (2, Cout, 2 * H, 2 * H)).double()
    ax = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, padding=1)
    wd = _dgrad_weights(w, None, True).double()                       # (16, Cin, Cout), tap 4 r + s
    k = wd.reshape(4, 4, Cin, Cout).permute(2, 3, 0, 1)               # (Cin, Cout, 4, 4)
    aty = F.conv2d(F.pad(y, (1, 1, 1, 1)), k, stride=2)               # rows 2 i - 1 .. 2 i + 2
    lhs, rhs = (ax * y).sum().item(), (x * aty[..., :H, :H]).sum().item()
    assert abs(lhs - rhs) <= 1e-6 * abs(lhs), (lhs, rhs)              # float32 rounding of the summed taps


@pytest.mark.parametrize("S,out", [(256, 224), (384, 336), (16, 16), (12, 29)])
@pytest.mark.parametrize("n", [1, 3])
def test_bilinear_resize_bwd_matches_fp64_and_adjoint(S, out, n):
    """ the gather-form adjoint against fp64 autograd of F.interpolate (bilinear, align_corners=False), zeros in the
    padding channels, and <A x, y> == <x, A^T y> with the forward kernel as A.  Against fp64 the bar is 1e-4: the
    forward kernel (like torch's float path) computes the source coordinate (o + 0.5) S / out - 0.5 in fp32, so its
    interpolation weights are off by up to ~S 2^-24 (measured 2.5e-5 at 256 -> 224, 4.4e-5 at 384 -> 336); the
    backward takes the same weights, which the adjoint identity checks to fp32 rounding """
    from textocvp_amd import kernels as K
    Cs = 32
    x = rnd("bl.x", (n, 3, S, S)).double().requires_grad_(True)
    dy = rnd("bl.dy", (n, 3, out, out))
    F.interpolate(x, size=(out, out), mode="bilinear", align_corners=False).backward(dy.double())
    got = K.bilinear_resize_bwd(dy.to(DEV), (S, S), Cs)
    torch.cuda.synchronize()
    err = _rel(got[..., :3].permute(0, 3, 1, 2), x.grad)
    print(f"\n[pdec-bwd] resize adjoint {S} -> {out} n={n}: {err:.2e} against fp64 coordinates")
    assert err < 1e-4
    assert torch.equal(got[..., 3:].cpu(), torch.zeros(n, S, S, Cs - 3))
    xs = rnd("bl.xs", (n, S, S, Cs)).to(DEV)
    ax = K.bilinear_resize_nhwc_to_nchw(xs, 3, out, out)
    terms = ax.double() * dy.to(DEV).double()
    lhs, scale = terms.sum().item(), terms.abs().sum().item()
    rhs = (xs[..., :3].double() * got[..., :3].double()).sum().item()
    assert abs(lhs - rhs) <= 1e-6 * scale, (lhs, rhs, scale)          # relative to the sum of |terms| (cancellation)


@pytest.mark.parametrize("Ks", [1, 24, 30])
@pytest.mark.parametrize("N", [256, 576])
def test_slot_composite_bwd_matches_fp64(Ks, N):
    """ adjoint of the softmax_K(alpha) weighted feature sum into the 800-column head layout, padding zero """
    from textocvp_amd import kernels as K
    Fd, ld = 768, 800
    dec = rnd("sc.dec", (1, Ks, N, ld))
    dec[..., Fd] *= 6.0
    d64 = dec[..., :Fd + 1].double().requires_grad_(True)
    alpha = torch.softmax(d64[..., Fd], dim=1)
    dR = rnd("sc.dR", (1, N, Fd))
    (d64[..., :Fd] * alpha[..., None]).sum(1).backward(dR.double())
    ddec, masks = dec.to(DEV), None
    _, masks = K.slot_composite(ddec, feat_dim=Fd)
    got = K.slot_composite_bwd(dR.to(DEV), ddec, masks, Fd)
    torch.cuda.synchronize()
    err = _rel(got[..., :Fd + 1], d64.grad)
    print(f"\n[pdec-bwd] composite K={Ks} N={N}: {err:.2e}")
    assert err < 1e-5
    assert torch.equal(got[..., Fd + 1:].cpu(), torch.zeros(1, Ks, N, ld - Fd - 1))


@pytest.mark.parametrize("S,N,D", [(1, 256, 128), (24, 576, 128), (30, 256, 64), (5, 7, 256)])
def test_ln_bcast_bwd_matches_fp64(S, N, D):
    """ sum over the patches of the LayerNorm backward at slot + position """
    from textocvp_amd import kernels as K
    sl = rnd("ln.s", (S, D)).double().requires_grad_(True)
    pos = rnd("ln.p", (N, D), scale=0.3)
    gm, bt = rnd("ln.g", (D,), "uniform", 2.0), rnd("ln.b", (D,))
    dy = rnd("ln.dy", (S, N, D), scale=1e-8)
    F.layer_norm(sl[:, None, :] + pos.double(), (D,), gm.double(), bt.double(), 1e-5).backward(dy.double())
    got = K.ln_bcast_bwd(sl.detach().float().to(DEV), pos.to(DEV), gm.to(DEV), dy.to(DEV), 1e-5)
    torch.cuda.synchronize()
    err = _rel(got, sl.grad)
    print(f"\n[pdec-bwd] ln bcast S={S} N={N} D={D}: {err:.2e}")
    assert err < 2e-5


# ---------------------------------------------------------------------------------------------------------------
# the whole backward against fp64 autograd on the oracle decoder

def _model(Ks, img_size, family, seed=0):
    """ family "saturated": the configs[3] fixtures' weights ("undamped": a x12 alpha row of the head, sharp masks that
    saturate the softmax over slots); "synth": the same weights with the alpha row at its plain scale (soft masks) """
    from textocvp_amd.setup_model import default_dinosaur_params, setup_model
    model = setup_model(default_dinosaur_params(num_slots=Ks, img_size=img_size)).eval()
    synth.fill_module_(model.decoder, prefix="dino.decoder.", family="undamped", seed=seed)
    if family == "synth":
        head = model.decoder.mlp[-1]
        with torch.no_grad():
            head.weight[-1] /= 12.0
            head.bias[-1] /= 12.0
    return model


def _inputs(Ks, F_, img_size):
    slots = rnd("e2e.slots", (F_, Ks, 128), scale=0.6)
    targets = synth.synth_videos(1, F_, height=img_size, width=img_size, seed=5)[0]
    return slots, targets


def _gscale(targets):
    return 2.0 / targets.numel()


@torch.no_grad()
def _gpu_gates(dec, slots, fpc):
    """ ReLU masks of the decoder's forward on the kernels (same chunks as the backward): the fp64 reference takes
    them as its gates, so that a pre-activation within fp32 rounding of 0 does not flip between the two """
    from textocvp_amd import kernels as K
    F_, Ks, D = slots.shape
    N = dec.num_patches
    ln = dec.mlp[0]
    lins = [m for m in dec.mlp[1:] if isinstance(m, torch.nn.Linear)]
    from textocvp_amd.train.patch_decoder import PatchDecoderLoss
    pdl = PatchDecoderLoss.__new__(PatchDecoderLoss)
    pdl.dec = dec
    wpad, bpad = pdl._head(lins[-1])
    pos = dec.pos_embed.detach().reshape(N, D).contiguous()
    mlp, cnn = [[] for _ in lins[:-1]], None
    for f0 in range(0, F_, fpc):
        sl = slots[f0:f0 + fpc].to(DEV)
        nf = sl.shape[0]
        with K.gemm_precision(dec.mlp_precision):
            x = K.layer_norm(sl.reshape(nf * Ks, 1, D).expand(nf * Ks, N, D).contiguous(), ln.weight, ln.bias, ln.eps,
                             add=pos)
            for j, lin in enumerate(lins[:-1]):
                x = K.linear(x, lin.weight, lin.bias, act=K.ACT_RELU)
                mlp[j].append((x > 0).reshape(nf, Ks, N, -1).cpu())
            y = K.linear(x, wpad, bpad)
        recons, _ = K.slot_composite(y.reshape(nf, Ks, N, -1), feat_dim=dec.out_dim - 1)
        acts = []
        dec._render(recons, keep=acts)
        ms = [(a > 0).permute(0, 3, 1, 2).cpu() for a in acts[:-1]]
        cnn = ms if cnn is None else [torch.cat([a, b]) for a, b in zip(cnn, ms)]
    return [torch.cat(m) for m in mlp] + cnn


@contextmanager
def _relu_gates(gates):
    """ torch.relu inside the oracle: x where the GPU's mask is set, else 0 (a select, like torch.relu's backward: a
    non-finite gradient does not pass a closed gate), the masks taken in call order """
    orig, it = torch.relu, iter(gates)
    torch.relu = lambda x: torch.where(next(it).to(x.device), x, torch.zeros_like(x))
    try:
        yield
    finally:
        torch.relu = orig


def oracle_loss_grad(model, slots, targets, grad_scale, gates=None):
    """ sum (img - target)^2 and grad_scale/2 * its slot gradient, torch.autograd in float64 """
    from oracle.slot_rollout_oracle import mlp_patch_decoder
    sd = {k[len("decoder."):]: v.detach().cpu().double() for k, v in model.state_dict().items()
          if k.startswith("decoder.")}
    s = slots.double().requires_grad_(True)
    ctx = _relu_gates(gates) if gates is not None else nullcontext()
    with torch.enable_grad(), ctx:
        img, _, _ = mlp_patch_decoder(sd, s, model.decoder.image_size)
        sq = ((img - targets.double()) ** 2).sum()
        sq.backward()
    return sq.item(), s.grad * (grad_scale / 2.0)


def _frame_errors(got, ref):
    got = got.cpu().double()
    return [((got[f] - ref[f]).abs().max() / ref[f].abs().max()).item() for f in range(ref.shape[0])]


@pytest.mark.parametrize("Ks,img_size", [(7, 224), (24, 224), (24, 336)])
# (synth.py's "damped" and "xavier" families leave this decoder's image head without an active ReLU path for some frames:
# their slot gradient is exactly zero, on the kernels and in fp64 alike)
@pytest.mark.parametrize("family", ["synth", "saturated"])
@pytest.mark.parametrize("fpc", [None, 1])
def test_loss_and_slot_grad_matches_fp64_autograd(Ks, img_size, family, fpc):
    from textocvp_amd.train.patch_decoder import PatchDecoderLoss
    F_ = 2
    model = _model(Ks, img_size, family).to(DEV)
    slots, targets = _inputs(Ks, F_, img_size)
    loss = PatchDecoderLoss(model, frames_per_chunk=fpc)
    used = loss.chunk_frames(Ks)
    sq, ds = loss.loss_and_slot_grad(slots.to(DEV), targets.to(DEV), _gscale(targets))
    torch.cuda.synchronize()
    gates = _gpu_gates(model.decoder, slots, used)
    sq_ref, ref = oracle_loss_grad(model, slots, targets, _gscale(targets), gates)
    e_sq = abs(sq.item() - sq_ref) / sq_ref
    assert all(ref[f].abs().max() > 0 for f in range(F_))
    fe = _frame_errors(ds, ref)
    print(f"\n[pdec-bwd] Ks={Ks} {img_size} {family} frames/chunk={used}: sq {e_sq:.1e}, frame max {max(fe):.2e}")
    assert e_sq <= 1e-5, e_sq
    assert max(fe) <= 1e-4, fe


# ---------------------------------------------------------------------------------------------------------------
# edge cases

def _run(model, slots, targets, gs, fpc=None):
    from textocvp_amd.train.patch_decoder import PatchDecoderLoss
    sq, ds = PatchDecoderLoss(model, frames_per_chunk=fpc).loss_and_slot_grad(slots.to(DEV), targets.to(DEV), gs)
    torch.cuda.synchronize()
    return sq.cpu(), ds.cpu()


def test_zero_and_power_of_two_grad_scales():
    """ grad_scale 0: exactly zero gradient, same loss; 2^-60 / 2^40: the gradient scales by exactly that factor """
    model = _model(7, 224, "saturated").to(DEV)
    slots, targets = _inputs(7, 2, 224)
    sq1, ds1 = _run(model, slots, targets, 1.0)
    sq0, ds0 = _run(model, slots, targets, 0.0)
    assert torch.equal(ds0, torch.zeros_like(ds0)) and torch.equal(sq0, sq1)
    for e in (-60, 40):
        _, dsg = _run(model, slots, targets, 2.0 ** e)
        assert torch.equal(dsg, ds1 * 2.0 ** e), e


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_non_finite_target_stays_non_finite(bad):
    """ NaN / inf target pixels in frame 1 (one frame per chunk): frame 1's gradient is non-finite exactly where the fp64
    reference's is (ReLU gates are selects on both sides) and somewhere at all; frames 0 and 2 are those of a clean run """
    model = _model(7, 224, "saturated").to(DEV)
    slots, targets = _inputs(7, 3, 224)
    gs = _gscale(targets)
    _, clean = _run(model, slots, targets, gs, fpc=1)
    tb = targets.clone()
    tb[1, :, 100:124, 30:54] = bad
    sq, ds = _run(model, slots, tb, gs, fpc=1)
    _, ref1 = oracle_loss_grad(model, slots[1:2], tb[1:2], gs, _gpu_gates(model.decoder, slots[1:2], 1))
    fin = torch.isfinite(ds[1])
    print(f"\n[pdec-bwd] target {bad}: frame 1 non-finite {int((~fin).sum())} of {fin.numel()} "
          f"(reference {int((~torch.isfinite(ref1)).sum())})")
    assert not torch.isfinite(sq).all() and not fin.all()
    assert torch.equal(fin, torch.isfinite(ref1[0]))
    assert torch.equal(ds[0], clean[0]) and torch.equal(ds[2], clean[2])


@pytest.mark.parametrize("change", ["load_state_dict", "inplace_conv", "inplace_linear", "inplace_bn"])
def test_gradient_follows_decoder_weight_changes(change):
    """ after a first call the decoder weights change: the derived backward weights follow, bit for bit what a fresh
    model with the new weights computes """
    from textocvp_amd.train.patch_decoder import PatchDecoderLoss
    model = _model(7, 224, "saturated").to(DEV)
    slots, targets = _inputs(7, 2, 224)
    gs = _gscale(targets)
    loss = PatchDecoderLoss(model)
    _, before = loss.loss_and_slot_grad(slots.to(DEV), targets.to(DEV), gs)
    before = before.cpu()
    dec = model.decoder
    with torch.no_grad():
        if change == "load_state_dict":
            model.load_state_dict(_model(7, 224, "saturated", seed=1).state_dict())
        elif change == "inplace_conv":
            dec.conv_patch_decoder[2].conv.weight.mul_(-1.5)
        elif change == "inplace_linear":
            dec.mlp[3].weight.mul_(0.5)
        else:
            dec.conv_patch_decoder[0].block[1].weight.mul_(2.0)
    sq, ds = loss.loss_and_slot_grad(slots.to(DEV), targets.to(DEV), gs)
    fresh = _model(7, 224, "saturated").to(DEV)
    fresh.load_state_dict(model.state_dict())
    sq_f, ds_f = _run(fresh, slots, targets, gs)
    assert not torch.equal(ds.cpu(), before)
    assert torch.equal(ds.cpu(), ds_f) and torch.equal(sq.cpu(), sq_f)


def test_run_to_run_reproducible():
    """ two identical calls: bitwise identical loss and gradient (no atomics anywhere on the path) """
    model = _model(24, 224, "saturated").to(DEV)
    slots, targets = _inputs(24, 3, 224)
    a = _run(model, slots, targets, _gscale(targets), fpc=2)
    b = _run(model, slots, targets, _gscale(targets), fpc=2)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
