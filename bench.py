#!/usr/bin/env python
"""
bench.py -- predicted frames / second of the TextOCVP slot-rollout hot path on MI355X.

One "step" = one pass of the hot path over one batch of synthetic sequences:
    SAVi encode (20 frames) -> TextOCVP_CustomTF rollout (19 steps) -> decode (19 frames)
at BASELINE.json configs[1]: 30 slots, 64x64x3, 1 seed + 19 predicted frames.  Inputs and weights
are resident in HBM before the timed region.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--batch B] [--dump-outputs DIR]
                    [--full [--no-cpu-baseline] [--no-extra] [--no-legs]]

A plain run does only what the headline needs: set up, W warm-up steps, the K timed steps, the outputs of the last of
them if --dump-outputs is given, and the result line (metric, value, unit, ms_per_step, dtype, mean PSNR / SSIM).
Everything else the benchmark measures runs only with --full, after the headline's timed steps: the second timed region
(value_no_overlap, roofline), the per-kernel pass (rooflines), "extra" and the CPU baseline; --no-extra, --no-legs and
--no-cpu-baseline leave parts of it out.

--dump-outputs DIR: after the K timed steps of the reported value, rank 0 writes what the LAST of them computed -- every
tensor forward_eval returns, and the PSNR / SSIM rows of the metric step -- as DIR/<name>.npy (dump_outputs: at most
64 MB in all).  Inputs and weights are seeded, so two builds run with the same arguments can be compared output for output.

N > 1: one process per GPU.  Under torchrun (WORLD_SIZE set) this process IS one rank; otherwise
``--gpus N`` makes this process a launcher that starts N fresh worker processes (RANK / LOCAL_RANK /
WORLD_SIZE / MASTER_ADDR / MASTER_PORT in their environment) BEFORE anything touches the GPU and
waits for them -- it replaces the reference's nn.DataParallel wrap (base/baseEvaluator.py:142-145).
Every rank runs its own batches (weak scaling, no collective inside the rollout); the per-sequence
PSNR / SSIM rows are all-gathered ONCE at the end (RCCL).

Prints ONE JSON line on rank 0; with --full it also carries
  "roofline":     dominant kernel (decoder 5x5 conv) timed IN the timed region with HIP events,
  "rooflines":    that entry + predictor GEMM, predictor attention and the slot-attention iteration
                  (HBM-bound, GB/s), each timed with HIP events in one extra untimed pass,
  "cpu_baseline": the CPU oracle (oracle/, kind "port") on a bounded sample: warm-up + 5 timed reps,
  "extra":        the same measurement at the authors' evaluation batch (32 sequences per GPU), at 8 and at 1
                  (the latency of one sequence), plus two bounded legs on the driver's clock:
                  "config4"  = BASELINE configs[3] from pixels (ExtendedDINOSAUR ViT-B/14, 24 slots, 224x224,
                               TextOCVP_T5, 1 seed + 29 preds, 16 sequences), with the ViT / predictor GEMM roofline;
                  "train_c5" = BASELINE configs[4] (predictor training step at the configs[1] shapes: 32 sequences,
                               30 slots, 1 seed + 19 preds; 3 graph-replayed steps after capture), with the roofline
                               of the weight-gradient kernel from the eager warm-up step's HIP events.
  "value" is measured with the decoder overlapped with the rollout on a second HIP stream (same kernels, bit-identical
  results); "value_no_overlap" and every per-kernel roofline come from a second timed region of the same K steps
  without the overlap, so that a kernel's duration is its own.
"""

import argparse
import json
import os
import socket
import statistics
import subprocess
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

NUM_SLOTS, NUM_CONTEXT, NUM_PREDS, RES = 30, 1, 19, 64
FP32_MFMA_PEAK_TFLOPS = 157.3            # MI355X_MICROARCH.md, chip-level parameters
F16_MFMA_PEAK_TFLOPS = 2500.0            # dense f16 / bf16 MFMA (same table)
HBM_PEAK_GBPS = 8000.0                   # HBM3E spec (6.3 TB/s achievable, same guide)
CONV_GFLOP_PER_SLOT_IMAGE = 2 * RES * RES * 64 * 64 * 25 / 1e9   # 0.839: one 64->64 5x5 layer
PATH_GFLOP_PER_FRAME = 149.5             # reference algorithm, K=30

# matrix-pipe time per algorithmic product in units of one 16-bit MFMA product, and the peak it is priced on
CONV_MODES = {
    "f16x3": ("conv5x5_dec_f16x3_kernel (decoder 5x5 conv 64->64, split-fp16 operands: 3 f16 MFMA products "
              "per algorithmic product, fp32-class)", 3, F16_MFMA_PEAK_TFLOPS),
    "f16x3-wino": ("conv5x5_wino_f16x3_kernel (decoder 5x5 conv 64->64 as vertical Winograd F(4, 5) x five horizontal taps: "
                   "40 split-fp16 products per 4 output pixels instead of 100, 3 f16 MFMA products each, fp32-class)",
                   1.2, F16_MFMA_PEAK_TFLOPS),
    "bf16x3": ("conv5x5_bf16x3_kernel (decoder 5x5 conv 64->64, split-bf16 operands, 3 bf16 MFMA products per "
               "algorithmic product)", 3, F16_MFMA_PEAK_TFLOPS),
    "f16f8": ("conv5x5_f16f8_kernel (decoder 5x5 conv 64->64, hybrid split: f16 main product + two e4m3 cross "
              "products on the 32x32x64 scaled MFMA)", 2, F16_MFMA_PEAK_TFLOPS),
    "fp32": ("conv5x5_mfma_kernel<64,64> (decoder 5x5 conv, exact fp32 MFMA)", 1, FP32_MFMA_PEAK_TFLOPS),
}
GEMM_UNITS = {22: ("f16x3", 3), 2: ("bf16x3", 3), 3: ("bf16x6", 6)}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=int(os.environ.get("TOCVP_BENCH_BATCH", 256)),
                    help="sequences per GPU per step")
    ap.add_argument("--strong", action="store_true",
                    help="strong scaling: --batch is the GLOBAL batch, split evenly over the ranks (the semantics of the "
                         "reference's nn.DataParallel, base/baseEvaluator.py:142-145, which scatters ONE batch over its "
                         "devices); default: weak scaling, --batch sequences per GPU")
    ap.add_argument("--full", action="store_true",
                    help="after the headline's timed steps, also measure value_no_overlap and the rooflines, the other "
                         "batches, captions and configs of `extra` and the CPU baseline (default: the headline alone)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline")
    ap.add_argument("--no-extra", action="store_true", help="--full without the batch-32 / 8 / 1 lines, the per-kernel "
                                                           "pass and the config-4 / training legs")
    ap.add_argument("--no-legs", action="store_true", help="--full without the config-4 and training legs of `extra`")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the outputs of the last timed step as DIR/<name>.npy (at most 64 MB in all)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    return args


def log(msg):
    print(f"[bench] {msg}", file=sys.stderr, flush=True)


def per_rank_batch(args, world):
    """ sequences per rank and step: --batch itself (weak scaling) or its share of the global batch (--strong) """
    if not args.strong:
        return args.batch
    if args.batch % world:
        raise SystemExit(f"--strong: the global batch {args.batch} is not a multiple of {world} ranks")
    return args.batch // world


class ClockSampler:
    """
    Shader clock of the visible GPU while a timed region runs: a thread reads the amdgpu hwmon node ``freq1_input`` (sclk, Hz)
    every 5 ms.  The chip lowers its clock under its power limit, by a different amount on every box: a kernel's duration in
    CYCLES (avg_launch_ms x sclk) separates code changes from box-to-box clock spread (the driver saw 3.728 -> 3.739 ms on the
    dominant kernel across rounds 3-4 while builder boxes showed 3.60-3.83 ms for one tree).  ``None`` when the node is not readable.
    """

    def __init__(self, pci_bus_id=None):
        import glob
        self.path, self.samples, self._stop, self._thread = None, [], False, None
        nodes = sorted(glob.glob("/sys/class/drm/card*/device/hwmon/hwmon*/freq1_input"))
        if pci_bus_id is not None:
            want = f":{int(pci_bus_id):02x}:"
            hit = [n for n in nodes if want in os.path.realpath(os.path.dirname(os.path.dirname(os.path.dirname(n))))]
            nodes = hit or nodes
        self.power_path, self.power = None, []
        for n in nodes:
            try:
                int(open(n).read())
                self.path = n
                break
            except (OSError, ValueError):
                continue
        if self.path is not None:                      # board power next to it (microwatts), where the node exists
            for name in ("power1_average", "power1_input"):
                cand = os.path.join(os.path.dirname(self.path), name)
                try:
                    int(open(cand).read())
                    self.power_path = cand
                    break
                except (OSError, ValueError):
                    continue

    def start(self):
        if self.path is None:
            return
        import threading
        self.samples, self.power, self._stop = [], [], False

        def loop():
            while not self._stop:
                try:
                    self.samples.append(int(open(self.path).read()) / 1e6)
                    if self.power_path is not None:
                        self.power.append(int(open(self.power_path).read()) / 1e6)
                except (OSError, ValueError):
                    pass
                time.sleep(0.005)
        self._thread = threading.Thread(target=loop, daemon=True)
        self._thread.start()

    def stop(self):
        """ -> {"mean", "min", "max", "samples"} in MHz, or None """
        if self._thread is None:
            return None
        self._stop = True
        self._thread.join()
        self._thread = None
        if not self.samples:
            return None
        v = self.samples
        out = {"mean": round(sum(v) / len(v), 1), "min": round(min(v), 1), "max": round(max(v), 1), "samples": len(v),
               "source": self.path}
        if self.power:
            out["board_power_w"] = {"mean": round(sum(self.power) / len(self.power), 1), "max": round(max(self.power), 1)}
        return out


# ------------------------------------------------------------------------------------------------
# launcher: python bench.py --gpus N without torchrun
# ------------------------------------------------------------------------------------------------
def worker_env(rank, world, port, base=None):
    """ environment of worker ``rank`` (what torchrun would set); pure function, covered by a CPU test """
    env = dict(os.environ if base is None else base)
    env.update({"RANK": str(rank), "LOCAL_RANK": str(rank), "WORLD_SIZE": str(world),
                "LOCAL_WORLD_SIZE": str(world), "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port),
                "HSA_ENABLE_IPC_MODE_LEGACY": env.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"),
                "TOCVP_BENCH_WORKER": "1"})
    return env


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch_workers(n, argv=None, device_count=None, popen=subprocess.Popen):
    """
    Start ``n`` fresh worker processes of this script and wait for them.  The launcher itself never
    initialises the GPU (``torch.cuda.device_count()`` does not), and never exec()s.  Returns the exit code.
    """
    if device_count is None:
        import torch
        device_count = torch.cuda.device_count()
    # TOCVP_DIST_BACKEND=gloo is the single-GPU rehearsal of the multi-process path: ranks share devices
    if device_count < n and os.environ.get("TOCVP_DIST_BACKEND", "nccl") != "gloo":
        log(f"--gpus {n} but only {device_count} GPU(s) are visible")
        return 2
    argv = list(sys.argv[1:] if argv is None else argv)
    port = free_port()
    procs = [popen([sys.executable, os.path.abspath(__file__)] + argv, env=worker_env(r, n, port))
             for r in range(n)]
    codes = [p.wait() for p in procs]
    return max(abs(c) for c in codes)


# ------------------------------------------------------------------------------------------------
# the timed region every rank runs (real worker and the CPU stub of tests/test_sharding_cpu.py alike)
# ------------------------------------------------------------------------------------------------
def run_timed(step, inp, warmup, steps, fence, gather, reduce_max, before=None, after=None):
    """
    W untimed warm-up steps, then EXACTLY K steps bracketed by ``fence()`` (barrier + device synchronise) on both sides;
    the per-sequence metric rows of the K steps go through ``gather`` (the path's ONLY collective) inside the region;
    the elapsed time is the MAX over ranks (``reduce_max``).  Returns (seconds, whatever ``after()`` returns, rows).
    """
    for _ in range(warmup):
        step(inp)
    fence()
    if before is not None:
        before()
    metrics = []
    t0 = time.perf_counter()
    for _ in range(steps):
        metrics.append(step(inp))
    import torch
    gathered = gather(torch.cat(metrics, dim=0))
    fence()
    elapsed = time.perf_counter() - t0
    extra = after() if after is not None else None
    return reduce_max(elapsed), extra, gathered


DUMP_BUDGET_BYTES = 64 << 20


def dump_outputs(out_dir, arrays, budget=DUMP_BUDGET_BYTES):
    """
    Write every tensor of ``arrays`` (name -> tensor) as ``out_dir/<name>.npy``, float64 kept and everything else as
    float32.  Each array gets an equal share of ``budget`` bytes: one that fits is written whole in its own shape, a
    larger one as the 1-D sample of its flattened values at sorted indices drawn without replacement from a PCG64 stream
    seeded by the array's name -- the same elements on every run with the same shapes.  Returns {name: shape written}.
    """
    import numpy as np
    import torch
    os.makedirs(out_dir, exist_ok=True)
    share = budget // max(1, len(arrays)) - 256          # 256: room for the .npy header
    written = {}
    for name, t in arrays.items():
        flat = t.detach().reshape(-1)
        flat = flat if flat.dtype == torch.float64 else flat.float()
        cap = share // flat.element_size()
        if flat.numel() > cap:
            rng = np.random.Generator(np.random.PCG64(np.random.SeedSequence(zlib.crc32(name.encode()))))
            idx = np.sort(rng.choice(flat.numel(), cap, replace=False))
            a = flat[torch.from_numpy(idx).to(flat.device)].cpu().numpy()
        else:
            a = flat.reshape(t.shape).cpu().numpy()
        np.save(os.path.join(out_dir, f"{name}.npy"), a)
        written[name] = a.shape
    return written


def stub_main(args):
    """
    CPU rehearsal of a worker (TOCVP_BENCH_STUB=1, gloo): the SAME launcher, environment, rendezvous, timed-region
    protocol (run_timed), metric gather and rank-0 line as the real worker, with the hot path replaced by a
    deterministic stand-in that encodes (rank, step-local sequence, frame) in its metric rows.  No GPU, no model:
    it exists so that the first 8-GPU run cannot die in plumbing (tests/test_sharding_cpu.py).
    """
    import torch
    import torch.distributed as dist
    from textocvp_amd.evaluator import gather_metrics
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend="gloo")
    B = per_rank_batch(args, world)

    def step(_inp):
        time.sleep(0.002 * (1 + rank % 3))                          # ranks finish at different times
        seq = torch.arange(B, dtype=torch.float32).view(B, 1, 1)
        frame = torch.arange(NUM_PREDS, dtype=torch.float32).view(1, NUM_PREDS, 1)
        return (1000.0 * rank + 10.0 * seq + 0.01 * frame).expand(B, NUM_PREDS, 2).clone()

    def fence():
        if world > 1:
            dist.barrier()

    def reduce_max(elapsed):
        t = torch.tensor([elapsed], dtype=torch.float64)
        if world > 1:
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    elapsed, _, rows = run_timed(step, None, args.warmup, args.steps, fence, gather_metrics, reduce_max)
    fail = os.environ.get("TOCVP_BENCH_STUB_FAIL_RANK")
    if rank == 0:
        frames = world * B * NUM_PREDS * args.steps
        print(json.dumps({"metric": "predicted frames/sec (STUB: no model, launcher / rendezvous / gather rehearsal)",
                          "value": round(frames / elapsed, 2), "unit": "predicted frames/s", "n_gpus": world,
                          "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(1e3 * elapsed / args.steps, 2),
                          "higher_is_better": True, "scaling": "strong" if args.strong else "weak", "stub": True,
                          "global_batch": B * world,
                          "gathered_rows": int(rows.shape[0]),
                          "row_owner": [int(v) for v in (rows[:, 0, 0] // 1000).tolist()]}), flush=True)
    if world > 1:
        dist.destroy_process_group()
    if fail is not None and int(fail) == rank:
        sys.exit(7)                                                 # after the collectives: nobody hangs on this rank


# ------------------------------------------------------------------------------------------------
def host_cores():
    """ cores this process may really use: min(affinity mask, cgroup v2/v1 CPU quota) """
    cores = os.cpu_count() or 1
    try:
        cores = len(os.sched_getaffinity(0))
    except AttributeError:
        pass
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            cores = min(cores, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                cores = min(cores, max(1, q // per))
        except (OSError, ValueError):
            pass
    return cores


def cpu_baseline(savi, pred):
    """
    CPU oracle (port of the reference path, oracle/) on a bounded sample of the same workload:
    1 untimed warm-up sequence, then 5 timed repetitions of a 2-sequence batch (the
    survey saw a 79 s outlier on a noisy host, hence median AND min).
    """
    import torch
    from oracle import slot_rollout_oracle as O
    from textocvp_amd import synth
    cores = host_cores()
    torch.set_num_threads(cores)
    ssd = {k: v.detach().cpu() for k, v in savi.state_dict().items()}
    psd = {k: v.detach().cpu() for k, v in pred.state_dict().items()}
    nseq = int(os.environ.get("TOCVP_CPU_BASELINE_SEQS", 2))
    reps = int(os.environ.get("TOCVP_CPU_BASELINE_REPS", 5))
    videos = synth.synth_videos(nseq, NUM_CONTEXT + NUM_PREDS, seed=0)
    tokens, lengths = synth.synth_captions(nseq, max_len=12, seed=0)
    noise = synth.synth_noise(nseq, NUM_SLOTS, 128, seed=1)
    times = []
    with torch.no_grad():
        O.forward_eval(ssd, psd, videos[:1], tokens[:1], lengths[:1], noise[:1], NUM_CONTEXT, NUM_PREDS)
        for _ in range(reps):
            t0 = time.perf_counter()
            O.forward_eval(ssd, psd, videos, tokens, lengths, noise, NUM_CONTEXT, NUM_PREDS)
            times.append(time.perf_counter() - t0)
    med, best = statistics.median(times), min(times)
    return {"value": round(nseq * NUM_PREDS / med, 3), "unit": "predicted frames/s", "cores": cores,
            "kind": "port", "value_best": round(nseq * NUM_PREDS / best, 3),
            "rep_seconds": [round(t, 2) for t in times],
            "sample": f"{reps} timed repetitions of one batch of {nseq} sequences (30 slots, 1 seed + 19 preds, "
                      f"64x64) after a 1-sequence warm-up; value = median ({med:.1f} s), value_best = min "
                      f"({best:.1f} s); torch-CPU fp32 oracle, {cores} threads"}


def arithmetic_string(savi, pred, kernels):
    attn = "f16x3 (split fp16 operands)" if kernels._ATTN_QK16 else "exact fp32 MFMA"
    return (f"fp32 storage / accumulation, operands split into 16-bit planes on the matrix cores: decoder convs "
            f"{savi.decoder.conv_precision}, predictor GEMMs {pred.predictor.gemm_precision}, encoder convs "
            f"{savi.encoder.conv_precision}, encoder / kv GEMMs {savi.encoder_gemm_precision}, attention "
            f"QK^T and PV {attn}; slot-attention iteration, softmax, LayerNorm, GRU exact fp32")


def leg_config4(dev, kernels, batch=64, reps=2):
    """
    BASELINE configs[3] on the driver's clock (reference 05_evaluate_predictor.py:53-104 on
    configs/models/ExtendedDINOSAUR.json): ExtendedDINOSAUR FROM PIXELS (DINOv2 ViT-B/14 backbone, 24 slots,
    224x224 -> 256 patches) + TextOCVP_T5, 1 seed + 29 preds, ``batch`` sequences (64 since the end of round 4: the rollout
    of 16 sequences is a chain of short kernels on 384 tokens per frame that neither fills the chip nor hides under the
    decoder -- 2053 / 2258 / 2344 frames/s at 16 / 32 / 64 sequences on one box); one warm-up, ``reps`` timed
    passes (median).  Roofline: the split-fp16 GEMM shape with the largest total time (ViT / MLP decoder /
    predictor), HIP events of the last timed pass.
    """
    import torch
    from textocvp_amd import synth
    from textocvp_amd.evaluator import forward_eval
    from textocvp_amd.setup_model import default_dinosaur_params, default_exp_params, setup_model, setup_predictor
    K4, P4 = 24, 29
    model = setup_model(default_dinosaur_params(num_slots=K4, img_size=224)).eval()
    exp = default_exp_params(num_slots=K4, num_context=1, num_preds=P4, predictor_name="TextOCVP_T5")
    pred = setup_predictor(exp).eval()
    synth.fill_module_(model, prefix="dino.")
    synth.fill_module_(pred, prefix="pred.")
    model, pred = model.to(dev), pred.to(dev)
    videos = synth.synth_videos(batch, 1 + P4, height=224, width=224, seed=4).to(dev)
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(1, 32000, (batch, 16), generator=g).to(dev)
    mask = torch.ones(batch, 16, dtype=torch.int64, device=dev)
    noise = synth.synth_noise(batch, K4, 128, seed=3).to(dev)
    times, timer = [], None
    with torch.no_grad():
        for it in range(1 + reps):
            if it == reps:
                kernels.TIMER = kernels.LaunchTimer(only=("gemm_split",))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = forward_eval(model, pred, videos, 1, P4, caption_tokens=ids, attn_masks=mask, init_noise=noise)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        timer, kernels.TIMER = kernels.TIMER, None
    assert bool(torch.isfinite(out["pred_imgs"]).all())
    med = statistics.median(times[1:])
    res = {"value": round(batch * P4 / med, 1), "unit": "predicted frames/s", "ms_per_step": round(1e3 * med, 1),
           "config": {"workload": "configs[3]: ExtendedDINOSAUR (DINOv2 ViT-B/14 from pixels) 24-slot 224x224 + "
                                  "MLPPatchDecoder + TextOCVP_T5, 1 seed + 29 preds", "batch_per_gpu": batch,
                      "num_slots": K4, "num_preds": P4, "resolution": 224},
           "timed": f"1 warm-up + {reps} passes of forward_eval (ViT encode 30 frames, slot attention, 29 rollout "
                    f"steps, decode 29 frames), median; the last pass carries HIP events on every split GEMM"}
    summ = {k: v for k, v in timer.summary().items() if v["launches"]}
    if summ:
        name, gk = max(summ.items(), key=lambda kv: kv[1]["total_ms"])
        tf = gk["units"] / gk["total_ms"] / 1e9
        res["roofline"] = {"bound": "mfma", "kernel": f"split-fp16 GEMM {name.split('_')[2]} (M x N x K), the shape "
                           f"with the largest total time of the pass", "achieved": round(tf, 1),
                           "peak": F16_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": round(tf / F16_MFMA_PEAK_TFLOPS, 4),
                           "matrix_units_per_product": 3, "frac_executed_mfma": round(3 * tf / F16_MFMA_PEAK_TFLOPS, 4),
                           "launches": gk["launches"], "avg_launch_ms": round(gk["total_ms"] / gk["launches"], 4),
                           "traffic": None}
    del model, pred, out, videos
    torch.cuda.empty_cache()
    return res


def leg_train(dev, kernels, batch=32, steps=3):
    """
    BASELINE configs[4] on the driver's clock (reference 04_train_predictor.py:57-108): one optimisation step of the
    TextOCVP_CustomTF predictor at the configs[1] shapes (``batch`` sequences, 30 slots, 1 seed + 19 preds, window
    10): frozen SAVi decomp -> BPTT rollout -> frozen decoder forward / backward -> clipped Adam.  One eager step with
    HIP events on the weight-gradient kernel (roofline), then graph capture, one replayed warm-up and ``steps`` timed
    graph-replayed steps.
    """
    import torch
    from textocvp_amd import synth
    from textocvp_amd.setup_model import default_exp_params, setup_model, setup_predictor
    from textocvp_amd.train.step import PredictorTrainStep
    exp = default_exp_params(num_slots=NUM_SLOTS, num_context=NUM_CONTEXT, num_preds=NUM_PREDS)
    savi, pred = setup_model(exp["model"]).eval(), setup_predictor(exp)
    synth.fill_module_(savi, prefix="savi.")
    synth.fill_module_(pred, prefix="pred.")
    ts = PredictorTrainStep(savi.to(dev), pred.to(dev))
    videos = synth.synth_videos(batch, NUM_CONTEXT + NUM_PREDS, seed=100).to(dev)
    tokens, lengths = synth.synth_captions(batch, max_len=12, seed=100)
    tokens, lengths = tokens.to(dev), lengths.to(dev)
    noise = synth.synth_noise(batch, NUM_SLOTS, 128, seed=200).to(dev)
    torch.cuda.reset_peak_memory_stats()
    kernels.TIMER = kernels.LaunchTimer(only=("gemm_tn",))
    first = ts.step(videos, tokens, lengths, init_noise=noise)               # eager, range-checked, HIP events
    torch.cuda.synchronize()
    timer, kernels.TIMER = kernels.TIMER, None
    ts.step_graphed(videos, tokens, lengths, init_noise=noise)               # eager step + capture of the two graphs
    float(ts.step_graphed(videos, tokens, lengths, init_noise=noise)["loss"])   # replayed warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = None
    for _ in range(steps):
        out = ts.step_graphed(videos, tokens, lengths, init_noise=noise)
    last = {k: round(float(v), 6) for k, v in out.items()}                   # reads the device-side snapshot
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    res = {"value": round(1.0 / dt, 3), "unit": "training steps/s", "ms_per_step": round(1e3 * dt, 1),
           "sequences_per_s": round(batch / dt, 1),
           "config": {"workload": "configs[4]: TextOCVP_CustomTF predictor training step (frozen SAVi, image + slot "
                                  "MSE, clip 0.05, Adam 1e-4), configs[1] shapes", "batch_per_gpu": batch,
                      "num_slots": NUM_SLOTS, "num_preds": NUM_PREDS, "resolution": RES},
           "timed": f"{steps} graph-replayed steps (forward + backward graph, optimiser graph) after one eager step, "
                    f"capture and one replayed warm-up", "first_eager_loss": round(float(first["loss"]), 6),
           "last": last, "peak_mem_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 1)}
    g = timer.summary().get("gemm_tn")
    if g and g["launches"]:
        tf = g["units"] / g["total_ms"] / 1e9
        from textocvp_amd.train import autograd as _ag
        split = _ag._WGRAD_PRECISION == "bf16x3"
        peak = 2500.0 if split else FP32_MFMA_PEAK_TFLOPS
        res["roofline"] = {"bound": "mfma",
                           "kernel": ("gemm_tn_bf16x3_kernel (weight gradients dW = dY^T X, split bf16 operands: 3 "
                                      "matrix products per algorithmic product, transposed LDS reads, split-K; the few "
                                      "launches whose row count is not a multiple of 32 run the exact-fp32 kernel)")
                           if split else "gemm_tn_f32_kernel (weight gradients dW = dY^T X, exact fp32 MFMA, split-K)",
                           "achieved": round(tf, 1), "peak": peak, "unit": "TFLOP/s", "frac": round(tf / peak, 4),
                           "matrix_units_per_product": 3 if split else 1,
                           "frac_executed_mfma": round((3 if split else 1) * tf / peak, 4),
                           "launches": g["launches"], "avg_launch_ms": round(g["total_ms"] / g["launches"], 4),
                           "ms_per_step": round(g["total_ms"], 1), "traffic": None,
                           "timed": "HIP events around every launch of the eager warm-up step of this run (graph "
                                    "replays cannot be bracketed per kernel)"}
    del ts, savi, pred
    torch.cuda.empty_cache()
    return res


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_workers(args.gpus))          # launcher: no GPU call before or after this line
    if os.environ.get("TOCVP_BENCH_STUB", "0") != "0":
        return stub_main(args)                        # CPU rehearsal of a worker (tests only)

    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the hot path has no CPU fallback")
    # one process per GPU; TOCVP_DIST_BACKEND=gloo lets several ranks share ONE GPU to rehearse the
    # multi-process path on a single-GPU box (the collective then runs on host copies of the metrics)
    backend = os.environ.get("TOCVP_DIST_BACKEND", "nccl")
    ndev = torch.cuda.device_count()
    if backend == "nccl" and world > ndev:
        raise SystemExit(f"WORLD_SIZE={world} ranks but only {ndev} GPU(s) visible")
    dev_index = local_rank % ndev
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend=backend)     # "nccl" is RCCL on ROCm

    from textocvp_amd import kernels, synth
    from textocvp_amd.evaluator import GraphedEval, forward_eval, gather_metrics
    from textocvp_amd.setup_model import default_exp_params, setup_model, setup_predictor

    exp = default_exp_params(num_slots=NUM_SLOTS, num_context=NUM_CONTEXT, num_preds=NUM_PREDS)
    savi = setup_model(exp["model"]).eval()
    pred = setup_predictor(exp).eval()
    synth.fill_module_(savi, prefix="savi.")
    synth.fill_module_(pred, prefix="pred.")
    savi, pred = savi.to(dev), pred.to(dev)

    def make_inputs(B, caption_len=12):
        videos = synth.synth_videos(B, NUM_CONTEXT + NUM_PREDS, seed=100 + rank).to(dev)
        tokens, lengths = synth.synth_captions(B, max_len=caption_len, seed=100 + rank)
        return videos, tokens.to(dev), lengths.to(dev), synth.synth_noise(B, NUM_SLOTS, 128, seed=200 + rank).to(dev)

    last = {} if args.dump_outputs else None          # --dump-outputs: what the latest step computed

    def step(inp, **kw):
        """ the hot path + the metric step after it: fused clamp + PSNR + SSIM kernel (tocvp_psnr_ssim_f32) """
        videos, tokens, lengths, noise = inp
        out = forward_eval(savi, pred, videos, NUM_CONTEXT, NUM_PREDS, caption_tokens=tokens,
                           caption_lengths=lengths, init_noise=noise, **kw)
        B, P, C, H, W = out["pred_imgs"].shape
        psnr, ssim = kernels.psnr_ssim(out["pred_imgs"].reshape(B * P, C, H, W),
                                       out["targets"].reshape(B * P, C, H, W), clamp01=True)
        if last is not None:
            last.update({k: v for k, v in out.items() if torch.is_tensor(v)}, psnr=psnr.view(B, P), ssim=ssim.view(B, P))
        return torch.stack([psnr.view(B, P), ssim.view(B, P)], dim=-1)        # (B, P, 2)

    def fence():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def metric_rows(out):
        B, P, C, H, W = out["pred_imgs"].shape
        psnr, ssim = kernels.psnr_ssim(out["pred_imgs"].reshape(B * P, C, H, W),
                                       out["targets"].reshape(B * P, C, H, W), clamp01=True)
        return torch.stack([psnr.view(B, P), ssim.view(B, P)], dim=-1)

    # small batches: the same step (hot path + metric kernel) replayed from a captured HIP graph -- from Python the
    # ~2400 short launches of a step are host-bound (evaluator.GraphedEval; bit-identical to the eager call)
    graphed = GraphedEval(savi, pred, NUM_CONTEXT, NUM_PREDS, epilogue=metric_rows,
                          overlap_decode=os.environ.get("TOCVP_GRAPH_OVERLAP", "0") != "0")

    def step_graphed(inp):
        videos, tokens, lengths, noise = inp
        return graphed(videos, caption_tokens=tokens, caption_lengths=lengths, init_noise=noise)["epilogue"].clone()

    def reduce_max(elapsed):
        t = torch.tensor([elapsed], device=dev if backend == "nccl" else "cpu", dtype=torch.float64)
        if world > 1:
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    def timed(inp, warmup, steps, timer_only=("conv5x5",), step=step, **kw):
        def start_timer():
            kernels.TIMER = kernels.LaunchTimer(only=timer_only)

        def stop_timer():
            timer, kernels.TIMER = kernels.TIMER, None
            return timer
        return run_timed(lambda i: step(i, **kw), inp, warmup, steps, fence, gather_metrics, reduce_max,
                         before=start_timer, after=stop_timer)

    B = per_rank_batch(args, world)
    inp = make_inputs(B)
    if rank == 0:
        log(f"world={world} batch/gpu={B} warmup={args.warmup} steps={args.steps}")
    # region 1 (the reported value): decoder overlapped with the rollout on a second HIP stream, no events.
    # region 2 (--full: value_no_overlap + the dominant kernel's roofline): the same K steps, serial order, HIP events
    # around the decoder convolutions only -- a kernel's duration is its own when nothing shares the chip.
    elapsed, _, all_metrics = timed(inp, args.warmup, args.steps, timer_only=(), overlap_decode=True)
    if last is not None:
        if rank == 0:
            shapes = dump_outputs(args.dump_outputs, last)
            log(f"outputs of the last timed step -> {args.dump_outputs}: {shapes}")
        last = None
    elapsed_no, timer, sclk = None, None, None
    if args.full:
        clock = ClockSampler(getattr(torch.cuda.get_device_properties(dev), "pci_bus_id", None)) if rank == 0 else None
        if clock is not None:
            clock.start()
        elapsed_no, timer, _ = timed(inp, 0, args.steps, overlap_decode=False)
        sclk = clock.stop() if clock is not None else None

    # Outside the timed region (rank 0): one pass with the decoder NOT overlapped with the rollout and EVERY
    # instrumented kernel bracketed by HIP events (thousands of event pairs would perturb the timed region).
    timer_all = None
    if rank == 0 and args.full and not args.no_extra:
        kernels.TIMER = kernels.LaunchTimer(only=("conv5x5", "gemm_", "mlp_fused_", "mha_", "slot_attn_"))
        step(inp, overlap_decode=False)
        torch.cuda.synchronize()
        timer_all, kernels.TIMER = kernels.TIMER, None

    extra = None
    if args.full and not args.no_extra:
        extra = {}
        notes = {32: "the authors' evaluation batch (scripts/05_evaluate_TextOCVP_CATER.sh)",
                 8: "small evaluation batch", 1: "one sequence: ms_per_step is the latency of 1 seed + 19 predicted "
                                                  "frames, encoder to metrics"}
        notes[256] = "twice the batch of rounds 1-4 (288 GB of HBM hold it easily: ~25 GB at this size): what larger shards buy"
        notes[128] = ("the headline batch of rounds 1-4 (kept for continuity: the default is 256 sequences per GPU since the "
                      "end of round 4, +1.5-2.3 % from the longer rounds of the rollout's kernels)")
        for b in (256, 128, 32, 8, 1):
            if b == B:
                continue
            n = max(2, args.steps) if b <= 32 else 2
            inp_b = make_inputs(b)
            el_eager, _, _ = timed(inp_b, 1, n)
            try:
                if world > 1:          # ranks must never diverge inside a collective: replay is a 1-GPU figure
                    raise RuntimeError("graph replay is timed on one GPU only")
                if b > 32:             # large batches are device-bound: eager only
                    raise RuntimeError("graph replay is a small-batch form")
                el, _, _ = timed(inp_b, 2, n, step=step_graphed)   # warm-up 1 captures, warm-up 2 replays
            except Exception as err:                              # a failed capture must not take the line with it
                if b <= 32:
                    log(f"graph replay at batch {b} failed ({type(err).__name__}: {err}); eager figure only")
                kernels.TIMER = None
                torch.cuda.synchronize()
                el = float("inf")
            best = min(el, el_eager)
            extra[f"batch_{b}"] = {"value": round(world * b * NUM_PREDS * n / best, 2), "unit": "predicted frames/s",
                                   "batch_per_gpu": b, "ms_per_step": round(1e3 * best / n, 2),
                                   "mode": "graph" if el <= el_eager else "eager",
                                   "ms_per_step_graph": round(1e3 * el / n, 2) if el != float("inf") else None,
                                   "ms_per_step_eager": round(1e3 * el_eager / n, 2),
                                   "note": notes[b] + "; graph: the step replayed from a captured HIP graph "
                                           "(evaluator.GraphedEval, serial decode); eager: launched from Python, "
                                           "decoder overlapped with the rollout on a second stream; value is the "
                                           "faster of the two (mode)"}
        graphed._graphs.clear()
        # the headline's caption has 12 tokens; the reference's text encoder admits 50 (text_encoders.py:36).  32-token
        # captions still take the collapsed cross-attention (32 caption slots per head, csrc/xattn.hip)
        inp_c = make_inputs(B, caption_len=32)
        n = min(max(2, args.steps), 5)          # bounded: a step of 256 sequences takes 1.2 s
        el_c, _, _ = timed(inp_c, 1, n)
        extra["caption_32"] = {"value": round(world * B * NUM_PREDS * n / el_c, 2), "unit": "predicted frames/s",
                               "batch_per_gpu": B, "ms_per_step": round(1e3 * el_c / n, 2), "caption_tokens": 32,
                               "vs_headline": round((world * B * NUM_PREDS * n / el_c) / (world * B * NUM_PREDS * args.steps / elapsed), 4),
                               "note": "configs[1] at the headline batch with 32-token captions (decoder overlapped, "
                                       "eager): the cross-attention of 17-32 token captions is collapsed over the caption "
                                       "like the 12-token one, with 32 caption slots per head"}
        del inp_c

    if rank == 0 and world == 1 and extra is not None and not args.no_legs:
        log("extra legs: configs[3] (ExtendedDINOSAUR from pixels) and configs[4] (training step) ...")
        for name, leg in (("config4", leg_config4), ("train_c5", leg_train)):
            t_leg = time.perf_counter()
            try:
                extra[name] = leg(dev, kernels)
                extra[name]["leg_seconds"] = round(time.perf_counter() - t_leg, 1)
            except Exception as err:                     # a failing leg must not take the headline line with it
                extra[name] = {"error": f"{type(err).__name__}: {err}"}
                kernels.TIMER = None

    if rank == 0:
        frames = world * B * NUM_PREDS * args.steps
        cp = savi.decoder.conv_precision
        if cp == "f16x3" and getattr(savi.decoder, "conv_wino", False):
            cp = "f16x3-wino"
        kernel_name, units, peak = CONV_MODES.get(cp, CONV_MODES["fp32"])
        rooflines = []
        roofline = None
        conv = timer.summary().get("conv5x5_64_64") if timer is not None else None
        if conv and conv["launches"]:
            avg_ms = conv["total_ms"] / conv["launches"]
            gflop_per_launch = CONV_GFLOP_PER_SLOT_IMAGE * conv["units"] / conv["launches"]
            achieved = gflop_per_launch / avg_ms            # GFLOP/ms == TFLOP/s
            traffic, traffic_from = None, None
            pmc = os.path.join(ROOT, "profiles", "conv_pmc_summary.json")
            if os.path.exists(pmc):
                with open(pmc) as f:
                    rec = json.load(f)
                # only a summary taken on the kernel that is running now counts
                if rec.get("slot_images_per_launch") and cp in rec.get("kernel", ""):
                    traffic = rec["hbm_bytes_per_launch"] * (
                        conv["units"] / conv["launches"]) / rec["slot_images_per_launch"]
                    traffic_from = "profiles/conv_pmc_summary.json (rocprofv3 PMC on scripts/decode_only.py, separate " \
                                   "FETCH_SIZE / WRITE_SIZE passes, gfx950 x2 fetch correction; launch-weighted mean of " \
                                   "the three instances the timed tree runs -- layer 1 collapsed input, layer 2 " \
                                   "activations in / out, layer 3 activations in + folded tail out; " \
                                   f"{rec.get('hbm_over_algorithmic', 0):.2f} x the algorithmic bytes; not this run)"
            roofline = {"bound": "mfma", "kernel": kernel_name,
                        "achieved": round(achieved, 2), "peak": peak, "unit": "TFLOP/s",
                        "frac": round(achieved / peak, 4),
                        "matrix_units_per_product": units,
                        "frac_executed_mfma": round(units * achieved / peak, 4),
                        "traffic": traffic, "traffic_from": traffic_from, "launches": conv["launches"],
                        "avg_launch_ms": round(avg_ms, 4), "gflop_per_launch": round(gflop_per_launch, 2),
                        # shader clock sampled during this region (amdgpu hwmon freq1_input) and the launch in CYCLES:
                        # the chip is power-limited on this kernel and boxes differ by several % in clock, not in cycles
                        "sclk_mhz": sclk,
                        "kcycles_per_launch": round(avg_ms * sclk["mean"], 1) if sclk else None,
                        "share_of_step_time": round(conv["total_ms"] / 1e3 / elapsed_no, 3),
                        "ceiling": (f"{units:g} executed matrix products per algorithmic product cap frac at {1.0 / units:.3f}; "
                                    "the bare v_mfma_f32_32x32x16_f16 loop sustains 1704 TFLOP/s on this chip under its power "
                                    f"limit (scripts/probes/mfma_shape_rate.hip) = {1704.0 / units:.0f} algorithmic = frac "
                                    f"{1704.0 / units / peak:.3f}: this kernel runs at {100.0 * achieved * units / 1704.0:.0f} % "
                                    "of that"),
                        "note": "achieved / avg_launch_ms are IN SITU (HIP events inside the second timed region: the "
                                "same K steps without the decode / rollout overlap, value_no_overlap; "
                                "algorithmic 0.839 GFLOP per slot image and layer, + 0.019 in the last layer, whose epilogue "
                                "also applies the decoder tail's taps); frac prices ALGORITHMIC flops (those of the "
                                "reference's direct convolution) against the dense f16 peak, frac_executed_mfma counts the "
                                "matrix products the kernel really issues (split arithmetic x 3, Winograd x 0.4)"}
            rooflines.append(roofline)
        if timer_all is not None:
            summ = timer_all.summary()

            def top(prefix):
                c = {k: v for k, v in summ.items() if k.startswith(prefix) and v["launches"]}
                return max(c.items(), key=lambda kv: kv[1]["total_ms"]) if c else (None, None)
            name, g = top("gemm_split")
            name_f, g_f = top("mlp_fused_")
            if g_f and (not g or g_f["total_ms"] >= g["total_ms"]):
                # the fused MLP (csrc/mlp_fused.hip) carries both products of an nn.Linear -> ReLU -> nn.Linear pair
                tf = g_f["units"] / g_f["total_ms"] / 1e9
                rooflines.append({"bound": "mfma", "kernel": "mlp_f16x3_fused_kernel, predictor MLP (f16x3) "
                                  f"{name_f[10:]} (M x E x hidden): relu(X W1^T + b1) W2^T + b2 + R in one launch, the "
                                  "hidden activation never leaves the CU; the GEMM-shaped kernel with the largest total "
                                  "time of the pass",
                                  "achieved": round(tf, 2), "peak": F16_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                                  "frac": round(tf / F16_MFMA_PEAK_TFLOPS, 4), "matrix_units_per_product": 3,
                                  "frac_executed_mfma": round(3 * tf / F16_MFMA_PEAK_TFLOPS, 4),
                                  "launches": g_f["launches"],
                                  "avg_launch_ms": round(g_f["total_ms"] / g_f["launches"], 4),
                                  "gflop_per_launch": round(g_f["units"] / g_f["launches"] / 1e9, 2),
                                  "traffic": None, "timed": "extra untimed pass, HIP events per launch"})
                try:                                   # PMC passes of scripts/mlp_fused_one.py, same row count only
                    rec = json.load(open(os.path.join(ROOT, "profiles", "mlp_pmc_summary.json")))
                    if str(rec["rows"]) == name_f[10:].split("x")[0]:
                        rooflines[-1]["traffic"] = rec["hbm_bytes_per_launch"]
                        rooflines[-1]["traffic_from"] = (
                            "profiles/mlp_pmc_summary.json (rocprofv3 PMC on scripts/mlp_fused_one.py, separate FETCH_SIZE / "
                            "WRITE_SIZE passes, gfx950 x2 fetch correction; bytes from beyond L2 -- the 8 MB of weight planes "
                            "and the X k-tiles are re-fetched per hidden chunk and mostly served by the Infinity Cache, not "
                            f"HBM; {rec['ratio']:.1f} x the algorithmic bytes; not this run)")
                except (OSError, KeyError, ValueError):
                    pass
            elif g:
                ns = int(name.split("_")[1][5:])
                mode, gu = GEMM_UNITS.get(ns, ("split", 3))
                tf = g["units"] / g["total_ms"] / 1e9
                rooflines.append({"bound": "mfma", "kernel": f"predictor GEMM ({mode}) "
                                  f"{name.split('_')[2]} (M x N x K), the shape with the largest total time: "
                                  "gemm_f16_planes_kernel where the activation arrives as fp16 operand planes (LayerNorm "
                                  "/ up-projection epilogue), gemm_bf16_wfrag_kernel (in-loop split) otherwise",
                                  "achieved": round(tf, 2), "peak": F16_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                                  "frac": round(tf / F16_MFMA_PEAK_TFLOPS, 4), "matrix_units_per_product": gu,
                                  "frac_executed_mfma": round(gu * tf / F16_MFMA_PEAK_TFLOPS, 4),
                                  "launches": g["launches"], "avg_launch_ms": round(g["total_ms"] / g["launches"], 4),
                                  "traffic": None, "timed": "extra untimed pass, HIP events per launch"})
            name, g = top("mha_")
            if g:
                tf = g["units"] / g["total_ms"] / 1e9
                au = 3 if kernels._ATTN_QK16 else 1
                apeak = F16_MFMA_PEAK_TFLOPS if kernels._ATTN_QK16 else FP32_MFMA_PEAK_TFLOPS
                aname = "mha_planes_kernel (q / k / v as fp16 operand planes from the projection's epilogue)" \
                    if kernels._ATTN_QK16 and kernels._MHA_PLANES else "mha_f32_kernel"
                rooflines.append({"bound": "mfma", "kernel": f"{aname}, predictor attention {name[4:]} "
                                  f"(B x heads x Tq x Tk x dh), QK^T + PV", "achieved": round(tf, 2),
                                  "peak": apeak, "unit": "TFLOP/s", "frac": round(tf / apeak, 4),
                                  "matrix_units_per_product": au, "frac_executed_mfma": round(au * tf / apeak, 4),
                                  "launches": g["launches"], "avg_launch_ms": round(g["total_ms"] / g["launches"], 4),
                                  "traffic": None, "timed": "extra untimed pass, HIP events per launch"})
            name, g = top("slot_attn_")
            if g:
                gbps = g["units"] / g["total_ms"] / 1e6
                rooflines.append({"bound": "hbm", "kernel": f"slot_attn kernel(s) of one slot-attention iteration "
                                  f"{name[10:]} (B x K x N x D): softmax over slots + weighted aggregation",
                                  "achieved": round(gbps, 1), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                                  "frac": round(gbps / HBM_PEAK_GBPS, 4), "launches": g["launches"],
                                  "avg_launch_ms": round(g["total_ms"] / g["launches"], 4),
                                  "bytes_per_launch": g["units"] / g["launches"],
                                  "traffic": None, "timed": "extra untimed pass, HIP events per iteration; "
                                  "algorithmic bytes = k and v (fp32) read once"})
        m = all_metrics.mean(dim=(0, 1))
        line = {
            "metric": "predicted frames/sec (1 seed, 19 preds, 64x64, 30 slots)",
            "value": round(frames / elapsed, 2), "unit": "predicted frames/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(1e3 * elapsed / args.steps, 2),
            "higher_is_better": True, "scaling": "strong" if args.strong else "weak", "vs_baseline": None,
            "dtype": arithmetic_string(savi, pred, kernels),
            "data": "synthetic",
            "config": {"workload": "configs[1]: SAVi 30-slot 64x64 + TextOCVP_CustomTF predictor, "
                                   "1 seed + 19 preds (encode 20 frames, 19 rollout steps, "
                                   "decode 19 frames)",
                       "batch_per_gpu": B, "global_batch": B * world, "num_slots": NUM_SLOTS,
                       "num_preds": NUM_PREDS, "resolution": RES, "weights": "synthetic (synth.py)",
                       "sharding": f"sequences x{world}, 1 all-gather of the (N, 19, 2) PSNR / SSIM rows"},
            "path_tflops": round(frames * PATH_GFLOP_PER_FRAME / 1e3 / elapsed, 2),
            "mean_psnr": round(float(m[0].item()), 3), "mean_ssim": round(float(m[1].item()), 4),
            "gathered_rows": int(all_metrics.shape[0]),
        }
        if args.full:
            line.update({"value_no_overlap": round(frames / elapsed_no, 2),
                         "ms_per_step_no_overlap": round(1e3 * elapsed_no / args.steps, 2),
                         "roofline": roofline, "rooflines": rooflines})
        if extra:
            line["extra"] = extra
        if world == 1 and args.full and not args.no_cpu_baseline:
            log(f"GPU: {line['value']} frames/s; timing the CPU oracle (warm-up + 5 reps of 2 sequences) ...")
            line["cpu_baseline"] = cpu_baseline(savi, pred)
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
