"""
Decoder timing of the SAVi variants against the shipped configuration on one device: milliseconds per 2040 slot images
(68 frames x 30 slots) for the ``up2`` variant (k 5, 8 x 8 broadcast, x2 upsampling after every hidden block, 64 x 64
output) and for the shipped decoder (k 5, 64 x 64 broadcast), plus the device time of every convk launch of one up2
decode in TFLOP/s and as a fraction of the f16 dense matrix peak (2516.6 TFLOP/s).  FLOPs are those the kernel executes
(phase form: 4 (k // 2 + 1)^2 taps per source pixel), a split-fp16 product counted once.

    python scripts/savi_variants_timing.py [--iters 20] [--out profiles/savi_variants_timing.json]
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/savi_variants_timing.py --profile-up2   # one up2 decode
"""

import argparse
import copy
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from textocvp_amd import kernels as K  # noqa: E402
from textocvp_amd import synth  # noqa: E402
from textocvp_amd.setup_model import default_exp_params, setup_model  # noqa: E402

F16_PEAK_TFLOPS = 2516.6
FRAMES, SLOTS = 68, 30


def model(tag):
    exp = default_exp_params(num_slots=SLOTS)
    p = copy.deepcopy(exp["model"])
    if tag == "up2":
        p["model_params"]["decoder"]["decoder_params"].update(resolution=[8, 8], upsample=2)
    savi = setup_model(p).eval()
    synth.fill_module_(savi, prefix="savi.")
    return savi.cuda()


def time_decode(savi, slots, iters):
    with torch.no_grad():
        for _ in range(3):
            savi.decode(slots)
        torch.cuda.synchronize()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(iters):
            savi.decode(slots)
        stop.record()
        torch.cuda.synchronize()
    return start.elapsed_time(stop) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile-up2", action="store_true", help="one warm-up and one up2 decode, nothing else")
    args = ap.parse_args()
    slots = synth.synth_tensor("timing.slots", (FRAMES, SLOTS, 128), "normal").cuda()
    if args.profile_up2:
        savi = model("up2")
        with torch.no_grad():
            savi.decode(slots)
            torch.cuda.synchronize()
            savi.decode(slots)
            torch.cuda.synchronize()
        return
    res = {"slot_images": FRAMES * SLOTS, "device": torch.cuda.get_device_name(0)}
    for tag in ("shipped", "up2"):
        res[f"{tag}_decode_ms"] = time_decode(model(tag), slots, args.iters)
    res["up2_over_shipped"] = res["up2_decode_ms"] / res["shipped_decode_ms"]

    savi = model("up2")
    with torch.no_grad():
        savi.decode(slots)
        torch.cuda.synchronize()
        K.TIMER = K.LaunchTimer(only=("convk",))
        try:
            savi.decode(slots)
            torch.cuda.synchronize()
            summ = K.TIMER.summary()
        finally:
            K.TIMER = None
    res["up2_convs"] = {name: {"ms": v["total_ms"], "tflops": v["units"] / v["total_ms"] / 1e9,
                               "of_f16_peak": v["units"] / v["total_ms"] / 1e9 / F16_PEAK_TFLOPS}
                        for name, v in summ.items()}
    line = json.dumps(res, indent=1)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
