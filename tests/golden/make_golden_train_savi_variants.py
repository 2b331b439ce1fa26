"""
Golden vectors of the predictor training step on frozen SAVi variants (train_savi_<tag>.npz, tags of
make_golden_savi_variants.variant_cfg): the recipe of make_golden.py::train_fixtures on the reference's own SAVi of each
variant (synthetic weights of synth.fill_module_, BatchNorm running statistics of synth.fill_batchnorm_stats_) and
PredictorWrapper(TextOCVP_CustomTF) (04_train_predictor.py:57-108 without the optimiser): decomp under no_grad ->
rollout -> decode of ``pred_slots.clone()`` -> nn.MSELoss on images + nn.MSELoss on slots (weights 1 / 1) -> backward()
through torch.autograd, SAVi frozen, dropout inactive.  K = 7, B = 2, 1 seed + 2 preds.  Stored: both losses, the L2 norm
of every parameter gradient and three gradients (every 4th row / column of the large matrices).

Runs on the CPU in the build container, like make_golden.py:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_train_savi_variants.py [out_dir]
"""

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

from make_golden import FixedNoise  # noqa: E402
from make_golden_savi_variants import KS, VARIANTS, build_variant, image_size  # noqa: E402
from textocvp_amd import synth  # noqa: E402

B, P, SEED = 2, 2, 0
KEEP = ("predictor.mlp_out.weight", "predictor.pe.pe", "predictor.predictor.0.attn.q.weight")


def train_variant_fixtures(tag, out_dir):
    cfg, savi, wrapper = build_variant(tag, num_context=1, num_preds=P)
    wrapper.eval()
    for p_ in savi.parameters():
        p_.requires_grad_(False)
    H, W = image_size(cfg)
    videos = synth.synth_videos(B, 1 + P, height=H, width=W, seed=SEED)
    tokens, lengths = synth.synth_captions(B, max_len=10, seed=SEED)
    noise = synth.synth_noise(B, KS, 128, seed=SEED + 1)
    C = videos.shape[2]
    with torch.no_grad(), FixedNoise(noise):
        hist = savi(mode="decomp", x=videos, num_imgs=1 + P, decode=False, caption_tokens=tokens,
                    caption_lengths=lengths)["slot_history"]
    pred_slots = wrapper(hist, caption_tokens=tokens, caption_lengths=lengths)
    dec = savi(mode="decode", slots=pred_slots.clone().reshape(B * P, KS, 128))
    pred_imgs = dec["recons_imgs"].view(B, P, C, H, W)
    mse = torch.nn.MSELoss()
    l_img = mse(pred_imgs, videos[:, 1:1 + P])
    l_slot = mse(pred_slots, hist[:, 1:1 + P])
    (l_img + l_slot).backward()
    names, norms, full = [], [], {}
    for name, p_ in wrapper.named_parameters():
        g = torch.zeros_like(p_) if p_.grad is None else p_.grad
        names.append(name)
        norms.append(float(g.norm()))
        if name in KEEP:
            full["grad::" + name] = (g[::4, ::4] if g.dim() == 2 and g.numel() > 40000 else g).detach().numpy()
    assert len(full) == len(KEEP), sorted(full)
    np.savez(os.path.join(out_dir, f"train_savi_{tag}.npz"), loss_img=l_img.item(), loss_slot=l_slot.item(),
             names=np.array(names), grad_norms=np.array(norms, dtype=np.float64), tokens=tokens.numpy(),
             lengths=lengths.numpy(), **full)
    print(f"train_savi_{tag}: losses", l_img.item(), l_slot.item(), "params", len(names), "kept", sorted(full))


if __name__ == "__main__":
    torch.set_num_threads(8)
    out = sys.argv[1] if len(sys.argv) > 1 else HERE
    for tag in VARIANTS:
        train_variant_fixtures(tag, out)
