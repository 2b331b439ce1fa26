#!/usr/bin/env python
"""
Timing of the predictor TRAINING step (BASELINE configs[4]; reference 04_train_predictor.py:57-108 with the
defaults of CONFIG.py: batch 64, 1 seed + 9 preds, window 10, Adam 1e-4, clip 0.05) on synthetic batches:
frozen decomp -> BPTT rollout -> frozen decoder forward/backward -> clipped Adam.
  --model savi      SAVi (64 x 64) + TextOCVP_CustomTF (default)
  --model dinosaur  ExtendedDINOSAUR (ViT-B/14 backbone, MLPPatchDecoder + CNN image head, --img-size) + TextOCVP_T5;
                    defaults batch 32, 24 slots.  Also reports the eager split of one step: decomp, rollout BPTT
                    (+ slot loss, clipping, Adam) and the patch decoder's loss + backward.
  --savi-variant    a SAVi variant (up2, k3, bn_up2_128, k7_mixed) built from the committed
                    tests/golden/state_dict_manifest_savi_<tag>.json, at its own image size.  Also reports the eager split
                    of one step: decomp, rollout BPTT (+ slot loss, clipping, Adam), the generic decoder's loss +
                    backward, and the forward decode of the same frames.
One process per GPU; with torchrun the gradients are averaged by one flat all-reduce per step.

    python scripts/bench_train.py [--model savi] [--batch 64] [--slots 8] [--preds 9] [--steps 5] [--warmup 2]
    python scripts/bench_train.py --model dinosaur [--img-size 224] [--batch 32] [--slots 24]
    python scripts/bench_train.py --savi-variant up2 [--batch 64] [--slots 8]
"""
import argparse
import copy
import json
import os
import sys
import time

import torch
import torch.distributed as dist

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from textocvp_amd import synth                                                        # noqa: E402
from textocvp_amd.setup_model import (default_dinosaur_params, default_exp_params, setup_model,   # noqa: E402
                                      setup_predictor)
from textocvp_amd.train.step import PredictorTrainStep                                # noqa: E402


def eager_split(ts, model, videos, tokens, lengths, noise, extra, a):
    """ ms of one eager step and of its two frozen-model parts timed alone (same shapes): decomp, and the patch
    decoder's loss + backward; the rest is the rollout BPTT with the slot loss, clipping and Adam """
    def timed(fn, n=3):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / n
    nc, P = 1, a.preds
    step = timed(lambda: ts.step(videos, tokens, lengths, init_noise=noise, **extra))
    with torch.no_grad():
        decomp = timed(lambda: model(mode="decomp", x=videos, num_imgs=nc + P, decode=False, init_noise=noise))
        hist = model(mode="decomp", x=videos, num_imgs=nc + P, decode=False, init_noise=noise)["slot_history"]
    slots = hist[:, nc:].reshape(a.batch * P, a.slots, -1).contiguous()
    tgt = videos[:, nc:nc + P].reshape(a.batch * P, *videos.shape[2:]).contiguous()
    dec = timed(lambda: ts.decoder.loss_and_slot_grad(slots, tgt, 2.0 / tgt.numel()))
    out = {"step": round(step, 1), "decomp": round(decomp, 1), "rollout_bptt_and_optimiser": round(step - decomp - dec, 1)}
    if a.savi_variant:
        with torch.no_grad():
            fwd = timed(lambda: model.decode(slots))
        return {**out, "decoder_loss_and_backward": round(dec, 1), "decoder_forward_decode": round(fwd, 1),
                "backward_over_forward": round(dec / fwd, 2), "decoder_frames_per_chunk": ts.decoder.chunk_frames(a.slots)}
    return {**out, "patch_decoder_loss_and_backward": round(dec, 1),
            "patch_decoder_frames_per_chunk": ts.decoder.chunk_frames(a.slots)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=("savi", "dinosaur"), default="savi")
    ap.add_argument("--img-size", type=int, default=224, help="ExtendedDINOSAUR image size (multiple of 14)")
    ap.add_argument("--savi-variant", choices=("up2", "k3", "bn_up2_128", "k7_mixed"), default=None,
                    help="SAVi variant of tests/golden/state_dict_manifest_savi_<tag>.json (with --model savi)")
    ap.add_argument("--batch", type=int, default=None, help="default 64 (savi) / 32 (dinosaur)")
    ap.add_argument("--slots", type=int, default=None, help="default 8 (savi) / 24 (dinosaur)")
    ap.add_argument("--preds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--eager", action="store_true", help="issue every launch from Python instead of replaying "
                                                         "the captured HIP graphs")
    a = ap.parse_args()
    dino = a.model == "dinosaur"
    a.batch = a.batch or (32 if dino else 64)
    a.slots = a.slots or (24 if dino else 8)
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0")) % torch.cuda.device_count()   # gloo rehearsal: ranks share a GPU
    torch.cuda.set_device(local)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(os.environ.get("TOCVP_DIST_BACKEND", "nccl"), rank=rank, world_size=world)
    dev = torch.device("cuda", local)
    if dino:
        exp = default_exp_params(num_slots=a.slots, num_context=1, num_preds=a.preds, predictor_name="TextOCVP_T5")
        savi = setup_model(default_dinosaur_params(num_slots=a.slots, img_size=a.img_size)).eval()
        synth.fill_module_(savi, prefix="dino.", family="undamped")
        res = a.img_size
    elif a.savi_variant:
        with open(os.path.join(ROOT, "tests", "golden", f"state_dict_manifest_savi_{a.savi_variant}.json")) as f:
            model_params = copy.deepcopy(json.load(f)["model_params"])
        model_params["num_slots"] = a.slots
        exp = default_exp_params(num_slots=a.slots, num_context=1, num_preds=a.preds)
        exp["model"]["model_params"] = model_params
        savi = setup_model(exp["model"]).eval()
        synth.fill_module_(savi, prefix="savi.")
        synth.fill_batchnorm_stats_(savi, prefix="savi.")
        res = model_params["encoder"]["encoder_params"]["resolution"][0]
    else:
        exp = default_exp_params(num_slots=a.slots, num_context=1, num_preds=a.preds)
        savi = setup_model(exp["model"]).eval()
        synth.fill_module_(savi, prefix="savi.")
        res = 64
    pred = setup_predictor(exp)
    synth.fill_module_(pred, prefix="pred.")
    ts = PredictorTrainStep(savi.to(dev), pred.to(dev))
    videos = synth.synth_videos(a.batch, 1 + a.preds, height=res, width=res, seed=100 + rank).to(dev)
    if dino:                                              # T5 token ids + attention masks (predictor_wrapper.py:101-111)
        gen = torch.Generator().manual_seed(100 + rank)
        tokens = torch.randint(1, 32000, (a.batch, 16), generator=gen).to(dev)
        lengths, extra = None, {"attn_masks": torch.ones(a.batch, 16, dtype=torch.int64, device=dev)}
    else:
        tokens, lengths = synth.synth_captions(a.batch, max_len=12, seed=100 + rank)
        tokens, lengths, extra = tokens.to(dev), lengths.to(dev), {}
    noise = synth.synth_noise(a.batch, a.slots, 128, seed=200 + rank).to(dev)

    def fence():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
    out = None
    run = ts.step if a.eager else ts.step_graphed
    for _ in range(a.warmup):
        out = run(videos, tokens, lengths, init_noise=noise, **extra)
    fence()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        out = run(videos, tokens, lengths, init_noise=noise, **extra)
    fence()
    dt = time.perf_counter() - t0
    split = eager_split(ts, savi, videos, tokens, lengths, noise, extra, a) if dino or a.savi_variant else None
    if rank == 0:
        print(json.dumps({
            "metric": "predictor training steps/s", "value": round(a.steps / dt, 3), "unit": "steps/s",
            "ms_per_step": round(1e3 * dt / a.steps, 1), "n_gpus": world,
            "launch_mode": "eager" if a.eager else "hip graphs (fwd+bwd, optimiser)",
            "sequences_per_s": round(world * a.batch * a.steps / dt, 1),
            "config": {"workload": ("TextOCVP_T5 training step, frozen ExtendedDINOSAUR" if dino else
                                    f"TextOCVP_CustomTF training step, frozen SAVi variant {a.savi_variant}"
                                    if a.savi_variant else "configs[4]: TextOCVP_CustomTF training step, frozen SAVi") +
                                   ", image + slot MSE, clipped Adam", "batch_per_gpu": a.batch, "num_slots": a.slots,
                       "num_preds": a.preds, "resolution": res},
            **({"eager_split_ms": split} if split else {}),
            "last": {k: round(float(v), 6) for k, v in out.items()},
            "peak_mem_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
