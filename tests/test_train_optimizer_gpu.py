"""
The optimiser half of the predictor training step against torch in float64: the clipped-Adam kernels called
through the C ABI (every element, every step, tails, null / NaN clip factors), PredictorTrainStep.apply over a
trajectory that crosses the warm-up and the cosine schedule, checkpoint round trips in this package's format
and in the reference trainer's (torch.optim.Adam) format, and the step following predictor weights that are
changed from outside (load_state_dict, load_checkpoint, in-place edits, assign=True).  Needs a real MI355X.

Sections 2-4 use a 2-layer TextOCVP predictor (every tensor kind of the 8-layer default, a quarter of its
51 M parameters) so that the fp64 CPU reference of every step stays cheap.
"""

import copy
import math
import types

import pytest
import torch
import torch.nn.functional as F

from textocvp_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24                      # unit round-off of fp32


def _L():
    from textocvp_amd import kernels as K
    return K.lib()


def _s():
    return torch.cuda.current_stream().cuda_stream


def _check(rc, name):
    from textocvp_amd import kernels as K
    K._check(rc, name)


def _hyper_fn(lr, warmup_steps, scheduler_steps, betas=(0.9, 0.999), eps=1e-8, eta_min=1e-7):
    """ PredictorTrainStep._hyper(t) of a step with these settings, without building one """
    from textocvp_amd.train.step import PredictorTrainStep
    cfg = types.SimpleNamespace(lr=lr, warmup_steps=warmup_steps, scheduler_steps=scheduler_steps, eta_min=eta_min,
                                betas=betas, eps=eps)
    cfg.lr_at = lambda it: PredictorTrainStep.lr_at(cfg, it)
    return lambda t: PredictorTrainStep._hyper(cfg, t)


# ---------------------------------------------------------------------------------------------------------------
# 1. the optimiser kernels through the C ABI
# ---------------------------------------------------------------------------------------------------------------
def _adam_ref_(p, m, v, g, h):
    """ torch.optim.Adam (no weight decay / amsgrad: exp_avg, exp_avg_sq, addcdiv with the bias corrections) in
    float64 on the scalars the kernel is given (h: the fp32 hyper vector) """
    lr, b1, b2, eps, bc1, bc2 = (float(x) for x in h)
    m.mul_(b1).add_((1.0 - b1) * g)
    v.mul_(b2).add_((1.0 - b2) * g * g)
    p.sub_((lr / bc1) * (m / (v.sqrt() / math.sqrt(bc2) + eps)))


@pytest.mark.parametrize("n", [1, 255, 257, 3 * 2 ** 20 + 5])
def test_adam_kernel_matches_fp64_adam_over_twelve_steps(n):
    """
    tocvp_adam_f32 over T = 12 launches with a new gradient each step and the scalars of PredictorTrainStep._hyper
    (warm-up of 2: step 1 runs at lr 0), against float64 Adam, every element of p, m and v after every step.
    Gradients span 1e-4 .. 10 per element; every 5th element sits at |g| ~ eps (bounded on its own).  Runs with
    gscale = NULL and with a device clip factor 0.37; the factor must give the same bits as a gradient scaled by
    0.37 beforehand.
    """
    T, lr = 12, 1e-3
    hyper = _hyper_fn(lr, warmup_steps=2, scheduler_steps=8)
    gen = torch.Generator().manual_seed(1000 + n)
    near = torch.arange(n) % 5 == 2
    mag = torch.pow(10.0, torch.empty(n, dtype=torch.float64).uniform_(-4.0, 1.0, generator=gen))
    mag[near] = 1e-8 * torch.pow(10.0, torch.empty(int(near.sum()), dtype=torch.float64).uniform_(-0.5, 0.5,
                                                                                                   generator=gen))
    grads = []
    for _ in range(T):
        sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0).double()
        grads.append((mag * sign * torch.empty(n, dtype=torch.float64).uniform_(0.5, 2.0, generator=gen)).float())
    p0 = ((torch.rand(n, generator=gen, dtype=torch.float64) * 2 - 1) * 2 ** -7).float()   # fp32 ulp of p << lr
    gs = torch.tensor([0.37], dtype=torch.float32)
    gs_dev = gs.to(DEV)

    runs = {k: [p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)] for k in ("null", "dev", "pre")}
    refs = {k: [p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)]
            for k in ("null", "dev")}
    gmax = {k: torch.zeros(n, dtype=torch.float64) for k in refs}
    pmax = {k: p0.double().abs() for k in refs}
    worst = {("null", False): 0.0, ("null", True): 0.0, ("dev", False): 0.0, ("dev", True): 0.0}
    for t in range(1, T + 1):
        h = torch.tensor(hyper(t), dtype=torch.float32)
        h_dev = h.to(DEV)
        g_dev = grads[t - 1].to(DEV)
        g_pre = g_dev * gs_dev                                   # fp32 product, rounded like the kernel's
        for key, g, scale in (("null", g_dev, None), ("dev", g_dev, gs_dev), ("pre", g_pre, None)):
            p, m, v = runs[key]
            _check(_L().tocvp_adam_f32(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, h_dev.data_ptr(),
                                       None if scale is None else scale.data_ptr(), _s()), "tocvp_adam_f32")
        for key, scale in (("null", 1.0), ("dev", float(gs))):
            g_ref = grads[t - 1].double() * scale
            _adam_ref_(*refs[key], g_ref, h)
            gmax[key] = torch.maximum(gmax[key], g_ref.abs())
            p, m, v = (x.cpu().double() for x in runs[key])
            pr, mr, vr = refs[key]
            pmax[key] = torch.maximum(pmax[key], pr.abs())
            assert ((v - vr).abs() <= 8 * t * U * vr).all(), (key, t, "exp_avg_sq")
            assert ((m - mr).abs() <= 8 * t * U * gmax[key]).all(), (key, t, "exp_avg")
            dp = (p - pr).abs()
            # beyond the fp32 rounding of p itself (half an ulp per step), in units of lr
            for grp in (False, True):
                sel = near == grp
                if not sel.any():
                    continue
                slack = (dp[sel] - t * U * pmax[key][sel]).max().item() / lr
                worst[(key, grp)] = max(worst[(key, grp)], slack)
                assert slack <= t * (2e-5 if not grp else 1e-4), (key, t, grp, slack)
        for a, b in zip(runs["dev"], runs["pre"]):             # the clip factor == scaling g beforehand, bit for bit
            assert torch.equal(a, b), t
    print(f"adam n={n}: worst |p - p_fp64| beyond fp32 rounding of p, in units of lr: "
          + ", ".join(f"{k}{' |g|~eps' if grp else ''} {w:.2e}" for (k, grp), w in worst.items()))


@pytest.mark.parametrize("nb", [1, 2, 7, 64, 255, 256])
def test_sqnorm_partials_and_column_sum_match_fp64(nb):
    """
    tocvp_sqnorm_partial_f32 with nblocks = nb over n below, at and above 256 nb (and a grid-stride multiple),
    then ag.colsum of the concatenated partials -- the route of PredictorTrainStep._clip_scale.  Ones count the
    elements of every partial exactly (a skipped, doubled or out-of-range element changes a count; the words after
    n hold 1e6); values of exponents 2^-60 .. 2^52 are held to the a-priori bound of the summation depth.
    """
    from textocvp_amd.train import autograd as ag
    sizes = [256 * nb - 1, 256 * nb, 256 * nb + 1, 3 * 256 * nb + 17]
    sizes = [n for n in sizes if n > 0]
    for n in sizes:
        buf = torch.full((n + 300,), 1e6, device=DEV)
        buf[:n] = 1.0
        part = torch.full((nb,), float("nan"), device=DEV)
        _check(_L().tocvp_sqnorm_partial_f32(buf.data_ptr(), part.data_ptr(), nb, n, _s()), "tocvp_sqnorm_partial_f32")
        counts = torch.bincount((torch.arange(n) // 256) % nb, minlength=nb).float()
        assert torch.equal(part.cpu(), counts), n
    gen = torch.Generator().manual_seed(nb)
    xs, parts = [], []
    for n in sizes:
        e = torch.randint(-60, 53, (n,), generator=gen).double()
        x = (torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0).double()
             * (1.0 + torch.rand(n, generator=gen, dtype=torch.float64)) * torch.pow(2.0, e)).float()
        xs.append(x)
        part = torch.full((nb,), float("nan"), device=DEV)
        xd = x.to(DEV)
        _check(_L().tocvp_sqnorm_partial_f32(xd.data_ptr(), part.data_ptr(), nb, n, _s()), "tocvp_sqnorm_partial_f32")
        parts.append(part)
    total = ag.colsum(torch.cat(parts).reshape(-1, 1))
    ref = sum(float((x.double() ** 2).sum()) for x in xs)
    rows = nb * len(sizes)
    chunk = 32 if rows >= 2048 else max(1, (rows + 63) // 64)
    depth = 1 + math.ceil(max(sizes) / (256 * nb)) + 8 + chunk + math.ceil(rows / chunk)
    err = abs(float(total.item()) - ref) / ref
    print(f"sqnorm nb={nb}: |sum - fp64| / sum = {err:.2e} (bound {depth * U:.1e})")
    assert err <= depth * U


_NAN, _INF = float("nan"), float("inf")


@pytest.mark.parametrize("max_norm", [0.05, 0.0])
@pytest.mark.parametrize("norm", [0.04, 0.05, 0.0625, 3.0, 0.0, _INF, _NAN])
def test_clip_scale_matches_clip_grad_norm(norm, max_norm):
    """
    tocvp_clip_scale_f32 against torch.nn.utils.clip_grad_norm_: norm below, at and above max_norm, a zero sum of
    squares, Inf and NaN; max_norm = 0 is clip=None (factor 1, no clipping).  A NaN norm gives a NaN factor (torch's
    clamp propagates it), and Adam with that factor turns every parameter into NaN, as torch.optim.Adam does after
    clip_grad_norm_.
    """
    sumsq = torch.tensor([norm * norm], dtype=torch.float32)
    out = torch.full((2,), 7.0, device=DEV)
    _check(_L().tocvp_clip_scale_f32(sumsq.to(DEV).data_ptr(), max_norm, out.data_ptr(), _s()), "tocvp_clip_scale_f32")
    got_c, got_n = (float(x) for x in out.cpu())
    # reference: clip_grad_norm_ on a one-element gradient of that norm
    p = torch.nn.Parameter(torch.zeros(1, dtype=torch.float64))
    p.grad = torch.tensor([math.sqrt(float(sumsq))], dtype=torch.float64)
    g0 = float(p.grad)
    if max_norm > 0:
        ref_n = float(torch.nn.utils.clip_grad_norm_([p], max_norm))
        ref_c = float(torch.clamp(max_norm / (torch.tensor(ref_n, dtype=torch.float64) + 1e-6), max=1.0))
        if math.isfinite(g0) and g0 > 0:                          # the factor clip_grad_norm_ applied
            assert float(p.grad) / g0 == pytest.approx(ref_c, rel=1e-12)
    else:
        ref_n, ref_c = math.sqrt(float(sumsq)), 1.0
    for got, ref in ((got_c, ref_c), (got_n, ref_n)):
        if math.isnan(ref):
            assert math.isnan(got)
        elif math.isinf(ref) or ref == 1.0 or ref == 0.0:
            assert got == ref
        else:
            assert got == pytest.approx(ref, rel=4 * U)

    # through Adam: finite gradients scaled by the factor
    g = torch.tensor([0.5, -1.0, 2.0], dtype=torch.float32)
    h = torch.tensor(_hyper_fn(1e-3, 0, 10)(1), dtype=torch.float32)
    pk, mk, vk = torch.ones(3, device=DEV), torch.zeros(3, device=DEV), torch.zeros(3, device=DEV)
    gd, hd = g.to(DEV), h.to(DEV)
    _check(_L().tocvp_adam_f32(pk.data_ptr(), gd.data_ptr(), mk.data_ptr(), vk.data_ptr(), 3, hd.data_ptr(),
                               out.data_ptr(), _s()), "tocvp_adam_f32")
    ref_p = [torch.nn.Parameter(torch.ones(3, dtype=torch.float64))]
    ref_p[0].grad = g.double() * ref_c
    torch.optim.Adam(ref_p, lr=float(h[0])).step()
    got_p = pk.cpu().double()
    assert torch.equal(torch.isnan(got_p), torch.isnan(ref_p[0].detach()))
    if math.isnan(ref_c):
        assert torch.isnan(got_p).all()
    else:
        assert (got_p - ref_p[0].detach()).abs().max().item() <= 1e-4 * float(h[0])


# ---------------------------------------------------------------------------------------------------------------
# 2, 3. PredictorTrainStep.apply over a trajectory; checkpoints
# ---------------------------------------------------------------------------------------------------------------
def _exp(Ks=7, P=2, predictor_name="TextOCVP_CustomTF", layers=2):
    from textocvp_amd.setup_model import default_exp_params
    exp = default_exp_params(num_slots=Ks, num_context=1, num_preds=P, predictor_name=predictor_name)
    exp["predictor"]["predictor_params"]["predictor_params"]["num_layers"] = layers
    return exp


def _fill_pred(pred, prefix="pred."):
    if type(pred.predictor).__name__ == "TextOCVP_T5":
        synth.fill_module_(pred.predictor.text_encoder, prefix="t5.")
        for part in ("predictor", "mlp_in", "mlp_out", "pe"):
            synth.fill_module_(getattr(pred.predictor, part), prefix=f"{prefix}predictor.{part}.")
    else:
        synth.fill_module_(pred, prefix=prefix)
    return pred


def _build_step(Ks=7, P=2, predictor_name="TextOCVP_CustomTF", prefix="pred.", savi=None, **opt):
    """ test_train_gpu._build_step with a 2-layer predictor and the optimiser settings of ``opt``; also returns
    the predictor's CPU copy before it moved to the device """
    from textocvp_amd.setup_model import setup_model, setup_predictor
    from textocvp_amd.train.step import PredictorTrainStep
    exp = _exp(Ks, P, predictor_name)
    if savi is None:
        savi = synth.fill_module_(setup_model(exp["model"]).eval(), prefix="savi.").to(DEV)
    pred = _fill_pred(setup_predictor(exp), prefix)
    cpu = copy.deepcopy(pred)
    kw = dict(lr=1e-4, clip=0.05, warmup_steps=0, text_dropout=0.0)
    kw.update(opt)
    ts = PredictorTrainStep(savi, pred.to(DEV), **kw)
    return ts, cpu


_OPT = dict(lr=1e-3, warmup_steps=2, scheduler_steps=6, eta_min=1e-7)
_SCALES = [3.0, 0.5, 2.0, 0.25, 6.0, 0.8, 1.5, 0.4, 4.0, 0.6]      # x clip: clipping on / off by turns


class _Grads:
    """ deterministic gradient sets: step t is cos(0.7 t) B1 + sin(0.7 t) B2 per tensor, scaled to a global norm
    of _SCALES[t] * 0.05; fp32, so the device and the fp64 reference see the same numbers """

    def __init__(self, shapes, seed=0):
        gen = torch.Generator().manual_seed(seed)
        self.b = {n: (torch.randn(s, generator=gen), torch.randn(s, generator=gen)) for n, s in shapes.items()}

    def __call__(self, t):
        c, s = math.cos(0.7 * t), math.sin(0.7 * t)
        raw = {n: c * b1 + s * b2 for n, (b1, b2) in self.b.items()}
        norm = math.sqrt(sum(float((x.double() ** 2).sum()) for x in raw.values()))
        k = _SCALES[t % len(_SCALES)] * 0.05 / norm
        return {n: (x * k).float() for n, x in raw.items()}


def _inject(ts, grads):
    for name, v in ts.model.names.items():
        v.grad = grads[name].to(DEV)


class _RefTrainer:
    """ the reference trainer's optimiser on float64 CPU copies: clip_grad_norm_ + torch.optim.Adam, lr from
    LRWarmUp + CosineAnnealingLR driven by WarmupVSScehdule with the 0-based iteration before the step (as restated
    in test_boundary_cpu.py::test_training_lr_schedule_matches_reference_driver) """

    def __init__(self, cpu_wrapper, lr, warmup_steps, scheduler_steps, eta_min, clip):
        self.wrapper = cpu_wrapper.double()
        self.named = dict(self.wrapper.named_parameters())
        self.opt = torch.optim.Adam(self.wrapper.parameters(), lr=lr)
        self.sched = torch.optim.lr_scheduler.CosineAnnealingLR(self.opt, T_max=scheduler_steps, eta_min=eta_min)
        self.lr0, self.W, self.clip = lr, warmup_steps if warmup_steps and warmup_steps > 0 else -1, clip
        self.active, self.iter_ = True, 0

    def step(self, grads):
        for name, p in self.named.items():
            p.grad = grads[name].double() if name in grads else None
        ps = [p for p in self.named.values() if p.grad is not None]
        if self.clip:
            norm = float(torch.nn.utils.clip_grad_norm_(ps, self.clip))
        else:
            norm = float(torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(p.grad) for p in ps])))
        if self.active:
            if self.iter_ > self.W:
                self.active = False
            elif self.iter_ >= 0:
                for g in self.opt.param_groups:
                    g["lr"] = self.lr0 * (self.iter_ / self.W)
        else:
            self.sched.step()
        lr = self.opt.param_groups[0]["lr"]
        self.opt.step()
        self.iter_ += 1
        return norm, lr

    def moments(self, name):
        st = self.opt.state[self.named[name]]
        return st["exp_avg"], st["exp_avg_sq"]


def _compare_with_ref(ts, ref, t, lr0, worst):
    """ weights of every trainable tensor after t steps: fp32 rounding of p (half an ulp per step) + 5e-5 lr per
    step for the update (the fp32 beta2 alone moves it by ~1e-5); moments to 3e-5 of the tensor's maximum """
    for name, v in ts.model.names.items():
        pr = ref.named[name].detach()
        p = v.data.cpu().double()
        slack = ((p - pr).abs() - t * U * pr.abs()).max().item() / lr0
        worst[0] = max(worst[0], slack)
        assert slack <= t * 5e-5, (name, t, slack)
        m, vv = (x.cpu().double() for x in ts.state[name])
        mr, vr = ref.moments(name)
        for got, r, what in ((m, mr, "exp_avg"), (vv, vr, "exp_avg_sq")):
            e = (got - r).abs().max().item() / max(r.abs().max().item(), 1e-30)
            worst[1] = max(worst[1], e)
            assert e <= 3e-5, (name, t, what, e)


@pytest.mark.parametrize("clip", [0.05, None])
def test_apply_follows_clipped_adam_trajectory(clip):
    """
    PredictorTrainStep.apply over 10 injected gradient sets against clip_grad_norm_ + torch.optim.Adam in float64:
    warm-up of 2 (step 1 at lr 0), the warm-up -> cosine boundary, cosine annealing down to eta_min, clipping active
    and inactive by turns (or clip=None).  Weights, moments and the returned (grad norm, lr) after every step.
    """
    ts, cpu = _build_step(clip=clip, **_OPT)
    ref = _RefTrainer(cpu, clip=clip, **_OPT)
    grads = _Grads({n: tuple(v.data.shape) for n, v in ts.model.names.items()})
    worst, worst_n, clipped = [0.0, 0.0], 0.0, set()
    for t in range(1, len(_SCALES) + 1):
        g = grads(t)
        _inject(ts, g)
        norm, lr = ts.apply()
        ref_norm, ref_lr = ref.step(g)
        assert lr == pytest.approx(ref_lr, rel=1e-9, abs=1e-15), t
        worst_n = max(worst_n, abs(norm - ref_norm) / ref_norm)
        assert abs(norm - ref_norm) <= 1e-5 * ref_norm, (t, norm, ref_norm)
        clipped.add(bool(clip) and ref_norm > clip)
        _compare_with_ref(ts, ref, t, _OPT["lr"], worst)
    assert ts.iteration == len(_SCALES)
    assert clipped == ({True, False} if clip else {False})
    print(f"apply, clip={clip}: worst weight error beyond fp32 rounding {worst[0]:.2e} lr; moments {worst[1]:.2e} "
          f"of max; grad norm {worst_n:.2e} relative")


def test_own_checkpoint_resumes_bit_for_bit(tmp_path):
    """ 3 steps, state_dict() -> torch.save; a fresh step on other weights (which has taken a step of its own)
    resumes through setup_model.load_checkpoint(only_model=False); both continue 4 steps on the same gradients:
    weights, Adam moments, iteration and lr equal the uninterrupted run's bit for bit """
    from textocvp_amd.setup_model import load_checkpoint
    ts1, _ = _build_step(**_OPT)
    grads = _Grads({n: tuple(v.data.shape) for n, v in ts1.model.names.items()}, seed=1)
    for t in range(1, 4):
        _inject(ts1, grads(t))
        ts1.apply()
    path = tmp_path / "ckpt.pth"
    torch.save(ts1.state_dict(epoch=4), path)
    ts2, _ = _build_step(prefix="predB.", savi=ts1.savi, **_OPT)
    _inject(ts2, grads(9))
    ts2.apply()
    out = load_checkpoint(str(path), ts2.wrapper, only_model=False, optimizer=ts2)
    assert out[1] is ts2 and out[4] == 5 and ts2.iteration == 3
    for name, v in ts1.model.names.items():
        assert torch.equal(ts2.model.names[name].data, v.data), name
    for t in range(4, 8):
        g = grads(t)
        _inject(ts1, g)
        _inject(ts2, g)
        r1, r2 = ts1.apply(), ts2.apply()
        assert r1 == r2, t
    assert ts1.iteration == ts2.iteration == 7
    assert set(ts1.state) == set(ts2.state) == set(ts1.model.names)
    for name, v in ts1.model.names.items():
        assert torch.equal(ts2.model.names[name].data, v.data), name
        assert torch.equal(ts2.state[name][0], ts1.state[name][0]) and torch.equal(ts2.state[name][1], ts1.state[name][1])
    sd1, sd2 = ts1.optimizer_state_dict(), ts2.optimizer_state_dict()
    assert sd1["param_groups"][0]["lr"] == sd2["param_groups"][0]["lr"]


def test_reference_optimizer_checkpoints_both_directions_with_frozen_t5(tmp_path):
    """
    TextOCVP_T5 (frozen T5 encoder inside wrapper.parameters()): a checkpoint whose optimizer_state_dict comes
    from torch.optim.Adam after 3 steps, without an ``iteration`` key (the reference's save_checkpoint), resumes
    through load_checkpoint -> load_training_state: every moment lands on its parameter by torch's index over ALL
    parameters, and 4 more steps follow the torch trajectory.  Then the other way: ts.optimizer_state_dict() loads
    into torch.optim.Adam over the CPU wrapper's parameters and one more step agrees.
    """
    from textocvp_amd.setup_model import load_checkpoint
    ts, cpu = _build_step(predictor_name="TextOCVP_T5", **_OPT)
    frozen = [n for n in ts.model.all_names if n not in ts.model.names]
    assert frozen and ts.model.all_names == [n for n, _ in cpu.named_parameters()]
    ref = _RefTrainer(cpu, clip=0.05, **_OPT)
    grads = _Grads({n: tuple(v.data.shape) for n, v in ts.model.names.items()}, seed=2)
    for t in range(1, 4):
        ref.step(grads(t))
    ckpt = {"epoch": 0, "model_state_dict": {k: v.float() if v.is_floating_point() else v
                                             for k, v in ref.wrapper.state_dict().items()},
            "optimizer_state_dict": ref.opt.state_dict(), "scheduler_state_dict": ref.sched.state_dict(),
            "lr_warmup": {"init_lr": _OPT["lr"], "warmup_steps": 2, "active": False, "final_step": 3}}
    path = tmp_path / "ref.pth"
    torch.save(ckpt, path)
    with torch.no_grad():                                   # the step starts elsewhere: the load must move it
        for v in ts.model.names.values():
            v.data.mul_(0.5)
    load_checkpoint(str(path), ts.wrapper, only_model=False, optimizer=ts)
    assert ts.iteration == 3 and set(ts.state) == set(ts.model.names)
    for name in ts.model.names:
        mr, vr = ref.moments(name)
        assert torch.equal(ts.state[name][0].cpu(), mr.float()), name
        assert torch.equal(ts.state[name][1].cpu(), vr.float()), name
    worst = [0.0, 0.0]
    for t in range(4, 8):
        g = grads(t)
        _inject(ts, g)
        norm, lr = ts.apply()
        ref_norm, ref_lr = ref.step(g)
        assert lr == pytest.approx(ref_lr, rel=1e-9, abs=1e-15) and abs(norm - ref_norm) <= 1e-5 * ref_norm, t
        _compare_with_ref(ts, ref, t, _OPT["lr"], worst)
    assert all(torch.equal(p.detach().cpu(), ref.named[n].detach().float())
               for n, p in ts.wrapper.named_parameters() if n in frozen)

    # this package's optimiser state -> torch.optim.Adam over every parameter of the CPU wrapper
    cpu2 = copy.deepcopy(ref.wrapper)
    with torch.no_grad():
        for n, p in cpu2.named_parameters():
            p.copy_(dict(ts.wrapper.named_parameters())[n].detach().cpu().double())
    opt = torch.optim.Adam(cpu2.parameters())
    opt.load_state_dict(ts.optimizer_state_dict())
    named2 = dict(cpu2.named_parameters())
    assert len(opt.state) == len(ts.model.names)
    for name in ts.model.names:
        st = opt.state[named2[name]]
        assert int(st["step"]) == ts.iteration
        assert torch.equal(st["exp_avg"], ts.state[name][0].cpu().double()), name
    g = grads(8)
    for n, p in named2.items():
        p.grad = g[n].double() if n in g else None
    torch.nn.utils.clip_grad_norm_([p for p in named2.values() if p.grad is not None], 0.05)
    for grp in opt.param_groups:
        grp["lr"] = ts.lr_at(ts.iteration)
    before = {n: p.detach().clone() for n, p in named2.items()}
    opt.step()
    _inject(ts, g)
    ts.apply()
    for name, v in ts.model.names.items():
        pr, p0 = named2[name].detach(), before[name]
        slack = ((v.data.cpu().double() - pr).abs() - U * pr.abs()).max().item() / _OPT["lr"]
        assert slack <= 5e-5, (name, slack)
        assert not torch.equal(pr, p0) or not g[name].any(), name


# ---------------------------------------------------------------------------------------------------------------
# 4. the step follows predictor weights changed from outside (full forward + backward)
# ---------------------------------------------------------------------------------------------------------------
class _Case:
    pass


@pytest.fixture(scope="module")
def weights_ab(tmp_path_factory):
    """ SAVi, one batch, predictor weights A and B, and the losses and gradients of a FRESH step on each """
    from textocvp_amd.setup_model import setup_model
    c = _Case()
    Ks, P = 7, 2
    exp = _exp(Ks, P)
    c.savi_cpu = synth.fill_module_(setup_model(exp["model"]).eval(), prefix="savi.")
    c.savi = copy.deepcopy(c.savi_cpu).to(DEV)
    c.videos = synth.synth_videos(2, 1 + P, seed=0)
    c.tokens, c.lengths = synth.synth_captions(2, max_len=12, lengths=[9, 12], seed=0)
    c.noise = synth.synth_noise(2, Ks, 128, seed=1)
    c.batch = (c.videos.to(DEV), c.tokens.to(DEV), c.lengths.to(DEV))
    c.others = {"init_noise": c.noise.to(DEV)}
    c.ref = {}
    for key, prefix in (("A", "pred."), ("B", "predB.")):
        ts, cpu = _build_step(prefix=prefix, savi=c.savi)
        setattr(c, f"sd_{key}", {k: v.clone() for k, v in cpu.state_dict().items()})
        c.ref[key] = _fresh_pass(ts, c)
        if key == "B":
            c.path_B = str(tmp_path_factory.mktemp("ckpt") / "B.pth")
            torch.save(ts.state_dict(), c.path_B)
    return c


def _fresh_pass(ts, c):
    losses = ts.loss_and_grads(*c.batch, **c.others)
    return losses, {n: v.grad.clone() for n, v in ts.model.names.items()}


def _assert_same_pass(losses, ts, ref, what, tol=2e-5):
    """ losses (to 1e-6) and every gradient of ``ts`` against a fresh step on the same weights.  Two fresh steps on
    the same weights differ by up to 1.6e-6 of a tensor's maximum (float atomics in the backward pass); planes of
    weights the step no longer holds move the slot loss alone by 2e-3 """
    ref_losses, ref_grads = ref
    for k in ("pred_slot_mse", "pred_img_mse"):
        assert abs(losses[k] - ref_losses[k]) <= 1e-6 * abs(ref_losses[k]), (what, k, losses[k], ref_losses[k])
    worst = 0.0
    for name, g in ref_grads.items():
        got = ts.model.names[name].grad
        e = (got - g).abs().max().item() / max(g.abs().max().item(), 1e-30)
        worst = max(worst, e)
        assert e <= tol, (what, name, e)
    print(f"{what}: worst gradient error {worst:.2e} of the tensor's maximum")


def _step_on(c):
    """ a new step on weights A after one pass, checked against the fresh reference on A """
    ts, _ = _build_step(savi=c.savi)
    _assert_same_pass(ts.loss_and_grads(*c.batch, **c.others), ts, c.ref["A"], "fresh step on A")
    return ts


def test_step_follows_load_state_dict(weights_ab):
    """ (a) wrapper.load_state_dict(sd_B) after a pass on A: the next pass equals a fresh step on B, and the CPU
    oracle differentiated by torch.autograd on B (as test_train_gpu's image-loss test) """
    from oracle import slot_rollout_oracle as O
    c = weights_ab
    ts = _step_on(c)
    ts.wrapper.load_state_dict(c.sd_B)
    losses = ts.loss_and_grads(*c.batch, **c.others)
    _assert_same_pass(losses, ts, c.ref["B"], "load_state_dict")

    B, P, Ks = 2, 2, 7
    savi_sd = {k: v.detach() for k, v in c.savi_cpu.state_dict().items()}
    sd = {k: v.detach().clone().requires_grad_(v.dtype.is_floating_point) for k, v in c.sd_B.items()}
    with torch.no_grad():
        hist = O.savi_decomp(savi_sd, c.videos, c.noise, 1 + P)
    preds = O.rollout(sd, hist, c.tokens, c.lengths, 1, P)
    imgs, _, _ = O.savi_decode(savi_sd, preds.reshape(B * P, Ks, 128), (64, 64), 3)
    l_img = F.mse_loss(imgs.view(B, P, 3, 64, 64), c.videos[:, 1:1 + P])
    l_slot = F.mse_loss(preds, hist[:, 1:1 + P])
    (l_img + l_slot).backward()
    assert abs(losses["pred_img_mse"] - l_img.item()) < 2e-4 * abs(l_img.item())
    assert abs(losses["pred_slot_mse"] - l_slot.item()) < 2e-4 * abs(l_slot.item())
    worst = 0.0
    for name, v in ts.model.names.items():
        r = sd[name].grad
        if r is None:
            assert v.grad.abs().max().item() == 0.0, name
            continue
        e = (v.grad.cpu().double() - r).abs().max().item() / max(r.abs().max().item(), 1e-30)
        worst = max(worst, e)
        assert e < 5e-3, (name, e)
    print(f"load_state_dict: worst gradient error against the oracle {worst:.2e}")


def test_step_follows_load_checkpoint(weights_ab):
    """ (b) setup_model.load_checkpoint(path_B, wrapper, only_model=False, optimizer=ts) after a pass on A """
    from textocvp_amd.setup_model import load_checkpoint
    c = weights_ab
    ts = _step_on(c)
    load_checkpoint(c.path_B, ts.wrapper, only_model=False, optimizer=ts)
    _assert_same_pass(ts.loss_and_grads(*c.batch, **c.others), ts, c.ref["B"], "load_checkpoint")


def test_step_follows_in_place_weight_edit(weights_ab):
    """ (c) mul_ of a few linear weights under torch.no_grad() after a pass on A == a fresh step on the edited
    weights """
    c = weights_ab
    edited = ["predictor.mlp_in.weight", "predictor.predictor.0.attn.q.weight",
              "predictor.predictor.1.cross_attention.mlp.0.weight", "predictor.mlp_out.weight"]
    ts = _step_on(c)
    params = dict(ts.wrapper.named_parameters())
    with torch.no_grad():
        for n in edited:
            params[n].mul_(1.5)
    sd_C = {k: v.clone() for k, v in c.sd_A.items()}
    for n in edited:
        sd_C[n].mul_(1.5)
    ref_ts, _ = _build_step(savi=c.savi)
    ref_ts.wrapper.load_state_dict(sd_C)
    ref_C = _fresh_pass(ref_ts, c)
    assert abs(ref_C[0]["loss"] - c.ref["A"][0]["loss"]) > 1e-3 * c.ref["A"][0]["loss"]   # the edit matters
    _assert_same_pass(ts.loss_and_grads(*c.batch, **c.others), ts, ref_C, "in-place mul_")


def test_step_follows_load_state_dict_assign(weights_ab):
    """ (d) load_state_dict(sd_B, assign=True) REPLACES the parameters: the step re-binds to the module's new tensors
    (pass equals a fresh step on B) and Adam then updates the tensors the module owns """
    c = weights_ab
    ts = _step_on(c)
    ts.wrapper.load_state_dict({k: v.to(DEV).clone() for k, v in c.sd_B.items()}, assign=True)
    _assert_same_pass(ts.loss_and_grads(*c.batch, **c.others), ts, c.ref["B"], "load_state_dict(assign=True)")
    name = "predictor.mlp_in.weight"
    p = dict(ts.wrapper.named_parameters())[name]
    before = p.detach().clone()
    ts.apply()
    assert ts.model.names[name].data.data_ptr() == p.data_ptr() and not torch.equal(p.detach(), before)


def test_graph_replay_and_eager_follow_weight_loads(weights_ab):
    """ (a) and (b) around captured graphs: replay after load_state_dict, eager after replay, and the eager step +
    re-capture after load_checkpoint, each against a fresh step on B """
    from textocvp_amd.setup_model import load_checkpoint
    c = weights_ab
    ts = _step_on(c)
    for _ in range(2):                                      # eager step + capture, then one replay
        dict(ts.step_graphed(*c.batch, **c.others))
    ref_losses, ref_grads = c.ref["B"]
    ref_norm = math.sqrt(sum(float((g.double() ** 2).sum()) for g in ref_grads.values()))

    ts.wrapper.load_state_dict(c.sd_B)                       # replay after load
    r = dict(ts.step_graphed(*c.batch, **c.others))
    _assert_same_pass(r, ts, c.ref["B"], "replay after load_state_dict")
    assert abs(r["grad_norm"] - ref_norm) <= 1e-5 * ref_norm

    ts.wrapper.load_state_dict(c.sd_B)                       # eager after replay (the replay's Adam moved the weights)
    _assert_same_pass(ts.loss_and_grads(*c.batch, **c.others), ts, c.ref["B"], "eager after replay")

    dict(ts.step_graphed(*c.batch, **c.others))              # replay
    load_checkpoint(c.path_B, ts.wrapper, only_model=False, optimizer=ts)
    _assert_same_pass(ts.loss_and_grads(*c.batch, **c.others), ts, c.ref["B"], "eager after replay + load_checkpoint")
    r = dict(ts.step_graphed(*c.batch, **c.others))          # eager step + re-capture (load_training_state)
    assert abs(r["loss"] - ref_losses["loss"]) <= 1e-6 * ref_losses["loss"]
    assert abs(r["grad_norm"] - ref_norm) <= 1e-5 * ref_norm
