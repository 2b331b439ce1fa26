"""
The predictor training step on a frozen ExtendedDINOSAUR (train/step.py with train/patch_decoder.py): the reference's
own training step as the golden (tests/golden/train_dino.npz, make_golden_train_dino.py: reference ExtendedDINOSAUR +
PredictorWrapper(TextOCVP_T5), 224 x 224, 7 slots, B = 2, 1 + 2 preds, torch.autograd), graph-replayed steps against
eager ones, the two-rank gradient average, and the bench shape (B = 32, 24 slots, 1 + 9).  Needs a real MI355X.
"""

import pytest
import torch

from textocvp_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
KS, B, P, SEED = 7, 2, 2, 91          # make_golden_train_dino.py


def rel_err(got, ref):
    ref = ref.double()
    return (got.detach().cpu().double() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-12)


def _build(Ks=KS, B_=B, P_=P, **kw):
    """ the golden's pair on this package (same synthetic weights as make_golden.py::build_reference_c4), the step,
    and the inputs of c4_inputs """
    from conftest import load_golden
    from textocvp_amd.setup_model import default_dinosaur_params, default_exp_params, setup_model, setup_predictor
    from textocvp_amd.train.step import PredictorTrainStep
    model = setup_model(default_dinosaur_params(num_slots=Ks, img_size=224)).eval()
    exp = default_exp_params(num_slots=Ks, num_context=1, num_preds=P_, predictor_name="TextOCVP_T5")
    pred = setup_predictor(exp).eval()
    synth.fill_module_(model, prefix="dino.", family="undamped")
    synth.fill_module_(pred, prefix="pred.")
    ts = PredictorTrainStep(model.to(DEV), pred.to(DEV), lr=1e-4, clip=0.05, warmup_steps=0, text_dropout=0.0, **kw)
    videos = synth.synth_videos(B_, 1 + P_, height=224, width=224, seed=SEED)
    if (Ks, B_, P_) == (KS, B, P):
        g = load_golden("train_dino.npz")
        ids, mask = torch.from_numpy(g["ids"]), torch.from_numpy(g["mask"])
    else:
        gen = torch.Generator().manual_seed(SEED)
        ids = torch.randint(1, 32000, (B_, 16), generator=gen)
        mask = torch.ones(B_, 16, dtype=torch.int64)
    noise = synth.synth_noise(B_, Ks, 128, seed=SEED + 1)
    return ts, videos, ids, mask, noise


def test_patch_decoder_is_selected():
    from textocvp_amd.train.patch_decoder import PatchDecoderLoss
    ts = _build()[0]
    assert isinstance(ts.decoder, PatchDecoderLoss)


def test_training_step_against_reference_golden():
    """ losses and gradients of the reference's own training step on ExtendedDINOSAUR (train_dino.npz); the bars of
    test_train_gpu.py::test_training_step_against_reference_golden """
    from conftest import load_golden
    g = load_golden("train_dino.npz")
    ts, videos, ids, mask, noise = _build()
    losses = ts.loss_and_grads(videos.to(DEV), ids.to(DEV), None, attn_masks=mask.to(DEV), init_noise=noise.to(DEV))
    e_img = abs(losses["pred_img_mse"] - float(g["loss_img"])) / float(g["loss_img"])
    e_slot = abs(losses["pred_slot_mse"] - float(g["loss_slot"])) / float(g["loss_slot"])
    print(f"\n[train-dino] losses img {losses['pred_img_mse']:.6g} ({e_img:.1e}) slot {losses['pred_slot_mse']:.6g} "
          f"({e_slot:.1e})")
    assert e_img < 2e-4 and e_slot < 2e-4
    worst = 0.0
    for name, ref_norm in zip(g["names"], g["grad_norms"]):
        v = ts.model.names.get(str(name))
        if v is None:                                     # frozen in the reference as here (the T5 encoder)
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
            ref = torch.from_numpy(g[key])
            assert rel_err(grad.reshape(ref.shape), ref) < 5e-3, key
    print(f"[train-dino] vs reference golden: worst gradient-norm error {worst:.2e}")


def test_graph_replayed_steps_equal_eager_steps():
    """ three optimiser steps eager and three graph-replayed (the first graphed call is the eager warm-up step) """
    res = []
    for graphed in (False, True):
        ts, videos, ids, mask, noise = _build()
        run = ts.step_graphed if graphed else ts.step
        res.append([dict(run(videos.to(DEV), ids.to(DEV), None, attn_masks=mask.to(DEV), init_noise=noise.to(DEV)))
                    for _ in range(3)])
    for a, b in zip(*res):
        assert abs(a["loss"] - b["loss"]) < 1e-5 * abs(a["loss"]) and a["lr"] == b["lr"]
        assert abs(a["grad_norm"] - b["grad_norm"]) < 1e-4 * abs(a["grad_norm"])
    assert res[0][0]["loss"] != res[0][2]["loss"]


def _ddp_worker(rank, world, port, out_dir):
    import os
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    ts, videos, ids, mask, noise = _build()
    sl = slice(rank, rank + 1)
    ts.loss_and_grads(videos[sl].to(DEV), ids[sl].to(DEV), None, attn_masks=mask[sl].to(DEV),
                      init_noise=noise[sl].to(DEV))
    ts.all_reduce_grads()
    if rank == 0:
        torch.save({n: v.grad.cpu() for n, v in ts.model.names.items() if v.grad is not None},
                   os.path.join(out_dir, "avg.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_gradient_average_equals_full_batch(tmp_path):
    """ two gloo ranks with one sequence each + the flat all-reduce == the gradient of the two-sequence batch """
    import socket
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_ddp_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    avg = torch.load(tmp_path / "avg.pt")
    ts, videos, ids, mask, noise = _build()
    ts.loss_and_grads(videos.to(DEV), ids.to(DEV), None, attn_masks=mask.to(DEV), init_noise=noise.to(DEV))
    for name, v in ts.model.names.items():
        if v.grad is None:
            continue
        assert rel_err(avg[name], v.grad.cpu()) < 2e-4, name


def test_bench_shape_step_is_finite():
    """ B = 32, 24 slots, 224 x 224, 1 + 9 (the reference CONFIG.py num_preds): finite losses and gradients """
    ts, videos, ids, mask, noise = _build(Ks=24, B_=32, P_=9)
    torch.cuda.reset_peak_memory_stats()
    out = ts.step(videos.to(DEV), ids.to(DEV), None, attn_masks=mask.to(DEV), init_noise=noise.to(DEV))
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() / 2 ** 30
    print(f"\n[train-dino] bench shape: loss {out['loss']:.6g} img {out['pred_img_mse']:.6g} "
          f"grad norm {out['grad_norm']:.4g}, peak {peak:.1f} GiB")
    assert all(torch.isfinite(torch.tensor(out[k])) for k in ("loss", "pred_img_mse", "pred_slot_mse", "grad_norm"))
    assert out["pred_img_mse"] > 0
    for name, v in ts.model.names.items():
        assert v.grad is not None and torch.isfinite(v.grad).all(), name
