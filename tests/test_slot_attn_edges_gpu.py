"""
Slot attention where a slot receives (almost) no attention, against float64 on the CPU.

The slot-attention iteration (csrc/slot_attn.hip) normalises the attention weights over LOCATIONS, after the softmax
over slots: a slot that wins no location has all of its weights near eps = 1e-8, and its update is still the (almost
uniform) mean of v.  The weights reach the matrix cores as fp16 planes, where such weights at a fixed scale are
subnormals with a few significant bits, so the test builds slots whose largest probability runs from ~1 down to 1e-11 and holds every slot's update to a bar
relative to that slot alone.  Both entry points (fp32 k / v rows and the fp16 k / v operand planes), a grid of
(slots, locations, batch) that reaches the multi-record ticket reduction and the single-record path, the module's
three iterations against the oracle, and the other attention kernels (mha, mha_planes, xattn_collapsed) on peaked
logits.
"""

import math
import os

import pytest
import torch

from oracle import slot_rollout_oracle as O
from textocvp_amd import kernels as K
from textocvp_amd import synth
from textocvp_amd.setup_model import default_exp_params, setup_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
D = 128
EPS = 1e-8
SLOT_BAR = 2e-6              # per slot: max_d |got - ref| <= SLOT_BAR * max_d |ref_slot|

KS = (1, 2, 7, 24, 30, 31, 32)
NS = (32, 96, 256, 576, 4096, 16384)
BS = (1, 3, 40, 300)
REGIMES = ("random", "graded", "one_winner", "q_zero", "single_slot")
MAX_ROWS = 300 * 576         # B * N of one case (the float64 reference runs on the CPU)


def _nrec(B, N):
    """ records (workgroups) per sample of csrc/slot_attn.hip pick_split """
    ntiles = N // 32
    want = max(1, 256 // max(B, 1))
    want = min(want, (ntiles + 3) // 4)
    tpw = (ntiles + 4 * want - 1) // (4 * want)
    return (ntiles + 4 * tpw - 1) // (4 * tpw)


def _grid():
    cases = []
    for i in range(24):
        regime = REGIMES[i % len(REGIMES)]
        Ks = 1 if regime == "single_slot" else KS[i % len(KS)]
        if regime in ("graded", "one_winner") and Ks < 4:
            Ks = KS[(i + 3) % len(KS)]
        N = NS[i % len(NS)]
        B = BS[i % len(BS)]
        if B * N > MAX_ROWS:
            B = max(b for b in BS if b * N <= MAX_ROWS)
        cases.append((regime, Ks, N, B))
    return cases


# slots moved against the keys' common component: their largest probabilities land near 3e-3, 1e-5 and 1e-11
GRADED_SHIFTS = (-0.6, -1.15, -3.0)


def _inputs(regime, Ks, N, B, seed):
    """ q (B, Ks, D), kv (B, N, 2 D) float32 on the CPU """
    g = torch.Generator().manual_seed(seed)
    m = torch.ones(D)                                                      # the keys' common component
    kk = torch.randn((B, N, D), generator=g) + m
    v = torch.randn((B, N, D), generator=g) + 0.3                          # every update bounded away from 0
    q = 0.5 * torch.randn((B, Ks, D), generator=g)
    if regime == "graded":
        extra = (-0.3, -2.0) if Ks >= 8 else ()
        shifts = extra + GRADED_SHIFTS
        for i, s in enumerate(shifts):
            q[:, Ks - len(shifts) + i] += s * m
    elif regime == "one_winner":
        q[:, 1:] += -3.5 * m
    elif regime == "q_zero":
        q.zero_()
    return q, torch.cat([kk, v], dim=-1).contiguous()


def _reference(q, kv, scale):
    """ float64: softmax over slots, + eps, normalised over locations, @ v -> (updates, attention) """
    q64, k64, v64 = q.double(), kv[..., :D].double(), kv[..., D:].double()
    attn = torch.softmax((q64 @ k64.transpose(1, 2)) * scale, dim=1) + EPS
    return (attn / attn.sum(-1, keepdim=True)) @ v64, attn


def _planes(kv):
    """ the fp16 operand planes of the fused kv projection: 2^8 x = hi + lo, (B, N, 2, 2 D) """
    X = kv * 256.0
    hi = X.half()
    return torch.stack([hi, (X - hi.float()).half()], dim=2).contiguous()


def _slot_errors(got, ref):
    """ per (sample, slot): max_d |got - ref| / max_d |ref| """
    err = (got.detach().cpu().double() - ref).abs().amax(-1)
    return err / ref.abs().amax(-1)


def _check_slots(got, ref, label):
    rel = _slot_errors(got, ref)
    worst = rel.amax(0)
    bad = (rel > SLOT_BAR).nonzero().tolist()
    msg = "; ".join(f"slot {s} rel {worst[s].item():.2e}" for s in sorted({s for _, s in bad}))
    assert not bad, f"{label}: {len(bad)} (sample, slot) updates above {SLOT_BAR:g} relative: {msg}"


def _check_attn(got, attn, q, kv, scale, label):
    """
    element-wise relative bar on the attention weights.  The logits are split fp16 products (~2^-22 relative per
    product) summed in fp32, so a logit is off by at most a few 2^-24 of L = scale * max sum_d |q_d k_d|; a weight
    p = exp(logit - max) / sum moves by that times two, plus the fp32 rounding of exp, the division and + eps.
    """
    L = (scale * (q.double().abs() @ kv[..., :D].double().abs().transpose(1, 2))).max().item()
    rel = 2.0 ** -20 * (L + 4.0)
    err = ((got.detach().cpu().double() - attn).abs() / attn).max().item()
    assert err <= rel, f"{label}: attention weight off by {err:.2e} relative (bar {rel:.2e}, logit bound {L:.1f})"


def test_grid_reaches_both_reductions():
    nrecs = [_nrec(B, N) for _, _, N, B in _grid()]
    assert any(n > 1 for n in nrecs) and any(n == 1 for n in nrecs)
    assert any(B > 128 for _, _, _, B in _grid()) and any(N < 128 and B < 128 for _, _, N, B in _grid())
    assert {Ks for _, Ks, _, _ in _grid()} == set(KS)
    assert {N for _, _, N, _ in _grid()} == set(NS)


@pytest.mark.parametrize("regime,Ks,N,B", _grid())
def test_slot_attn_edges_against_fp64(regime, Ks, N, B):
    scale = D ** -0.5
    q, kv = _inputs(regime, Ks, N, B, seed=1000 * Ks + N + B)
    ref, attn = _reference(q, kv, scale)
    slot_max = (attn - EPS).amax(-1).amax(0)                                # largest probability of each slot
    if regime == "graded":                                                  # the construction reaches every band
        assert (slot_max > 1e-3).any() and (slot_max < 1e-2).any()
        assert ((slot_max > 1e-6) & (slot_max < 1e-4)).any(), slot_max
        assert (slot_max < 1e-9).any(), slot_max
    if regime == "one_winner":
        assert (slot_max[1:] < 1e-9).all(), slot_max
    if regime == "q_zero":
        assert torch.allclose(attn, torch.full_like(attn, 1.0 / Ks + EPS), rtol=1e-15, atol=0)

    qd, kvd = q.to(DEV), kv.to(DEV)
    ws = K.slot_attn_workspace(B, N, DEV)
    a32 = torch.empty((B, Ks, N), device=DEV)
    got = K.slot_attn_iter(qd, kvd[..., :D], kvd[..., D:], scale, EPS, attn_out=a32, ws=ws)
    planes = _planes(kv).to(DEV)
    apl = torch.empty((B, Ks, N), device=DEV)
    got_p = K.slot_attn_iter_planes(qd, planes, scale, EPS, attn_out=apl, ws=ws)
    torch.cuda.synchronize()

    rel = _slot_errors(got, ref).amax(0)
    rel_p = _slot_errors(got_p, ref).amax(0)
    print(f"{regime} Ks={Ks} N={N} B={B} nrec={_nrec(B, N)}: worst slot rel err fp32 rows {rel.max().item():.2e}, "
          f"planes {rel_p.max().item():.2e}; slot max prob {slot_max.min().item():.1e}..{slot_max.max().item():.1e}")
    _check_slots(got, ref, f"slot_attn_iter {regime} Ks={Ks} N={N} B={B}")
    _check_slots(got_p, ref, f"slot_attn_iter_planes {regime} Ks={Ks} N={N} B={B}")
    _check_attn(a32, attn, q, kv, scale, "slot_attn_iter attn_out")
    _check_attn(apl, attn, q, kv, scale, "slot_attn_iter_planes attn_out")

    # deterministic: the same bits on a second call (the ticket reduction adds its records in a fixed order)
    assert torch.equal(K.slot_attn_iter(qd, kvd[..., :D], kvd[..., D:], scale, EPS, ws=ws), got)
    assert torch.equal(K.slot_attn_iter_planes(qd, planes, scale, EPS, ws=ws), got_p)


# ---- SlotAttention.iterate, three iterations, against the oracle in float64 -------------------------------------

def _module_inputs(sd, B, Ks, N, seed):
    """
    features sharing a common component and initial slots along the direction that raises / lowers q . k for it:
    in the first iteration slot Ks - 1 is empty (largest probability < 1e-8) and slot Ks - 2 near-empty (< 1e-3)
    """
    g = torch.Generator().manual_seed(seed)
    c = torch.randn(D, generator=g, dtype=torch.float64)
    feats = c + 0.5 * torch.randn((B, N, D), generator=g, dtype=torch.float64)
    x = O.layer_norm(feats, sd["norm_input.weight"], sd["norm_input.bias"], 1e-3)
    k0 = O.linear(x, sd["to_k.weight"], sd["to_k.bias"]).mean(dim=(0, 1))
    w = sd["norm_slot.weight"] * (sd["to_q.weight"].t() @ k0)
    w = (w - w.mean()) / (w - w.mean()).norm()
    a = torch.ones(Ks, dtype=torch.float64)
    a[Ks - 3], a[Ks - 2], a[Ks - 1] = 0.5, 0.0, -2.5
    slots = 10.0 * a[None, :, None] * w + torch.randn((B, Ks, D), generator=g, dtype=torch.float64)
    return feats.float(), slots.float()


@pytest.mark.parametrize("kv_planes,precision,N", [("1", None, 4096), ("0", None, 4096), ("1", "fp32", 4096),
                                                    ("1", None, 576)])
@torch.no_grad()
def test_slot_attention_module_with_empty_slots(kv_planes, precision, N, monkeypatch):
    monkeypatch.setenv("TOCVP_SA_KV_PLANES", kv_planes)
    B, Ks = 2, 7
    exp = default_exp_params(num_slots=Ks, num_context=1, num_preds=2)
    model = setup_model(exp["model"]).eval()
    synth.fill_module_(model, prefix="savi.")
    sa = model.slot_attention
    assert sa.kv_planes == (kv_planes == "1")
    assert sa.to_k.weight.shape[1] == D, "the test builds 128-wide features"
    sd = {n_: t.detach().double() for n_, t in sa.state_dict().items()}
    feats, slots0 = _module_inputs(sd, B, Ks, N, seed=N)

    ref, attn = O.slot_attention(sd, feats.double(), slots0.double(), 1, return_attn=True)
    slot_max = (attn - EPS).amax(-1).amax(0)
    assert slot_max[Ks - 1] < 1e-8 and slot_max[Ks - 2] < 1e-3 and slot_max[: Ks - 3].min() > 0.1, slot_max
    ref = O.slot_attention(sd, feats.double(), slots0.double(), 3)

    sa = sa.to(DEV)
    ctx = K.gemm_precision(precision) if precision else torch.no_grad()
    with ctx:
        kv = sa.project_kv(feats.to(DEV))
        got = sa.iterate(kv, slots0.to(DEV), 3)
    torch.cuda.synchronize()
    rel = _slot_errors(got, ref)
    print(f"SlotAttention.iterate planes={kv_planes} precision={precision or 'default'} N={N}: per-slot rel err "
          f"{[f'{e:.1e}' for e in rel.amax(0).tolist()]}")
    assert rel.max().item() <= 2e-5, rel.amax(0)


# ---- the other attention kernels on peaked logits ----------------------------------------------------------------

def _peaked_qk(B, H, Tq, Tk, dh, g):
    """
    q, k (B, T, H dh) whose logits (scale dh^-0.5) are peaked: for Tk <= dh the keys are orthogonal and q picks the
    logits outright -- one key per row dominates by 7..21 (the others at 1e-9..1e-3) or the spread runs to 30; for
    longer key sets q is a multiple of one key, so that key's logit sits ~16 above a N(0, 2) crowd
    """
    scale = dh ** -0.5
    if Tk <= dh:
        basis = torch.linalg.qr(torch.randn((B, H, dh, dh), generator=g, dtype=torch.float64))[0][..., :Tk]
        kh = basis.transpose(-1, -2) * math.sqrt(dh)                        # (B, H, Tk, dh), rows of norm sqrt(dh)
        dom = torch.randint(0, Tk, (B, H, Tq), generator=g)
        logits = 10.0 - (7.0 + 14.0 * torch.rand((B, H, Tq, Tk), generator=g, dtype=torch.float64))
        logits.scatter_(-1, dom[..., None], 10.0)
        spread = torch.rand((B, H, Tq, 1), generator=g, dtype=torch.float64) < 0.25
        logits = torch.where(spread, 30.0 * torch.rand((B, H, Tq, Tk), generator=g, dtype=torch.float64) - 15.0, logits)
        qh = (logits / scale) @ kh / dh                                       # q . k_j * scale == logits[j]
    else:
        kh = torch.randn((B, H, Tk, dh), generator=g, dtype=torch.float64)
        dom = torch.randint(0, Tk, (B, H, Tq), generator=g)
        beta = 16.0 / (dh * scale)
        qh = beta * torch.gather(kh, 2, dom[..., None].expand(B, H, Tq, dh))
    q = qh.permute(0, 2, 1, 3).reshape(B, Tq, H * dh).float()
    k = kh.permute(0, 2, 1, 3).reshape(B, Tk, H * dh).float()
    return q, k


def _check_rows(got, ref, tol, label):
    """ row-wise: max over the row of |got - ref| <= tol * max |ref row| """
    got = got.detach().cpu().double()
    err = (got - ref).abs().amax(-1)
    scale = ref.abs().amax(-1)
    worst = (err / scale).max().item()
    assert worst <= tol, f"{label}: worst row error {worst:.2e} of the row's max |out| (bar {tol:g})"
    return worst


ROW_BAR = 4e-6


@pytest.mark.parametrize("B,H,Tq,Tk,dh", [(2, 8, 70, 64, 64), (3, 4, 30, 20, 32), (2, 8, 300, 300, 64),
                                          (1, 8, 129, 40, 64)])
def test_mha_peaked_logits(B, H, Tq, Tk, dh):
    g = torch.Generator().manual_seed(B * 1000 + Tk)
    q, kk = _peaked_qk(B, H, Tq, Tk, dh, g)
    v = torch.randn((B, Tk, H * dh), generator=g) + 0.5
    ref = O.attention(q.double(), kk.double(), v.double(), H, dh ** -0.5)
    got = K.mha(q.to(DEV), kk.to(DEV), v.to(DEV), H, dh ** -0.5)
    w = _check_rows(got, ref, ROW_BAR, f"mha {B}x{H}x{Tq}x{Tk}x{dh}")
    # key_len = 1 on the first sample: every row of it is v of key 0 (one weight of 1)
    kl = torch.full((B,), Tk, dtype=torch.int32)
    kl[0] = 1
    pad = torch.arange(1, Tk + 1)[None, :] > kl.long()[:, None]
    ref1 = O.attention(q.double(), kk.double(), v.double(), H, dh ** -0.5, key_mask=pad)
    got1 = K.mha(q.to(DEV), kk.to(DEV), v.to(DEV), H, dh ** -0.5, key_len=kl.to(DEV))
    w1 = _check_rows(got1, ref1, ROW_BAR, f"mha key_len=1 {B}x{H}x{Tq}x{Tk}x{dh}")
    print(f"mha peaked {B}x{H}x{Tq}x{Tk}x{dh}: worst row error {w:.2e}, with key_len 1: {w1:.2e}")


def _planes_of(x2):
    X = torch.clamp(x2 * 256.0, -65504.0, 65504.0)
    hi = X.to(torch.float16)
    return torch.stack([hi, (X - hi.float()).to(torch.float16)], dim=1).contiguous()


@pytest.mark.skipif(os.environ.get("TOCVP_PRECISION") == "fp32" or os.environ.get("TOCVP_ATTN_QK") == "fp32",
                    reason="operand planes exist in the f16x3 arithmetic only")
@pytest.mark.parametrize("B,H,Tq,Tk", [(2, 8, 64, 64), (3, 8, 300, 300), (1, 6, 257, 257)])
def test_mha_planes_peaked_logits(B, H, Tq, Tk):
    dh, E = 64, H * 64
    g = torch.Generator().manual_seed(B * 7 + Tk)
    q, kk = _peaked_qk(B, H, Tq, Tk, dh, g)
    v = torch.randn((B, Tk, E), generator=g) + 0.5
    qp = K.SplitAct(_planes_of(q.reshape(B * Tq, E)).to(DEV), (B, Tq, E))
    kvp = K.SplitAct(_planes_of(torch.cat([kk, v], -1).reshape(B * Tk, 2 * E)).to(DEV), (B, Tk, 2 * E))
    kl = torch.full((B,), Tk, dtype=torch.int32)
    kl[B - 1] = 1
    pad = torch.arange(1, Tk + 1)[None, :] > kl.long()[:, None]
    ref = O.attention(q.double(), kk.double(), v.double(), H, dh ** -0.5, key_mask=pad)
    with K.gemm_precision("f16x3"):
        assert K.mha_planes_ok(H, E)
        got = K.mha_planes(qp, 0, kvp, 0, kvp, E, B, Tq, Tk, H, dh ** -0.5, key_len=kl.to(DEV))
    w = _check_rows(got, ref, ROW_BAR, f"mha_planes {B}x{H}x{Tq}x{Tk}")
    print(f"mha_planes peaked {B}x{H}x{Tq}x{Tk}: worst row error {w:.2e}")


@pytest.mark.parametrize("B,Tq,Lt,qgain", [(2, 70, 12, 14.0), (3, 100, 1, 8.0), (2, 64, 24, 16.0)])
@torch.no_grad()
def test_xattn_collapsed_peaked_logits(B, Tq, Lt, qgain):
    """ the query projection scaled by ``qgain``: logit spreads of ~30 over the caption; Lt = 1 is one key """
    from textocvp_amd.models.Blocks.attention import TransformerDecoderBlock
    E, H, dh = 512, 8, 64
    blk = TransformerDecoderBlock(embed_dim=E, head_dim=dh, kv_dim=E, num_heads=H, mlp_size=2048).eval()
    g = torch.Generator().manual_seed(B * 100 + Lt)
    for n_, p_ in blk.named_parameters():
        if p_.dim() > 1:
            p_.copy_((torch.rand(p_.shape, generator=g) * 2 - 1) * p_.shape[1] ** -0.5)
        else:
            p_.copy_((1.0 if "weight" in n_ else 0.0) + (torch.rand(p_.shape, generator=g) * 2 - 1) * 0.2)
    blk.cross_attn.q.weight.mul_(qgain)
    x = torch.randn((B, Tq, E), generator=g)
    text = torch.randn((B, Lt, E), generator=g)
    P64 = {n_: p_.detach().double() for n_, p_ in blk.named_parameters()}
    ln = torch.nn.functional.layer_norm
    qn = ln(x.double(), (E,), P64["ln_cross_att_q.weight"], P64["ln_cross_att_q.bias"], 1e-6)
    tn = ln(text.double(), (E,), P64["ln_cross_att_kv.weight"], P64["ln_cross_att_kv.bias"], 1e-6)
    q = (qn @ P64["cross_attn.q.weight"].t()).view(B, Tq, H, dh).transpose(1, 2)
    kk = (tn @ P64["cross_attn.k.weight"].t()).view(B, Lt, H, dh).transpose(1, 2)
    vv = (tn @ P64["cross_attn.v.weight"].t()).view(B, Lt, H, dh).transpose(1, 2)
    logits = q @ kk.transpose(-1, -2) * dh ** -0.5
    if Lt > 1:
        spread = (logits.amax(-1) - logits.amin(-1)).max().item()
        assert spread > 20, spread
    att = (torch.softmax(logits, dim=-1) @ vv).transpose(1, 2).reshape(B, Tq, E)
    y_ref = att @ P64["cross_attn.out_projection.weight"].t() + P64["cross_attn.out_projection.bias"]
    blk = blk.to(DEV)
    xd = x.to(DEV)
    with K.gemm_precision("f16x3"):
        tkv = blk.project_text(text.to(DEV))
        assert tkv.collapsed is not None and tkv.collapsed[2] == Lt
        Gf, Hf, _ = tkv.collapsed
        lnq = blk.ln_cross_att_q
        z = K.xattn_collapsed(xd, lnq.weight, lnq.bias, lnq.eps, Gf, Hf, blk.cross_attn.out_projection.bias, H, Lt,
                              dh ** -0.5)
    # the attention half alone (z - x), row-wise against its own magnitude
    w = _check_rows(z.cpu().double() - x.double(), y_ref, 2e-5, f"xattn_collapsed B={B} Tq={Tq} Lt={Lt}")
    print(f"xattn_collapsed peaked B={B} Tq={Tq} Lt={Lt}: worst row error {w:.2e}")
