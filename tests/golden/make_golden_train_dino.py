"""
Golden vector of the predictor training step on a frozen ExtendedDINOSAUR (train_dino.npz): the recipe of
make_golden.py::train_fixtures on the reference's own ExtendedDINOSAUR and PredictorWrapper(TextOCVP_T5)
(04_train_predictor.py:57-108 without the optimiser): decomp under no_grad -> rollout -> decode on
``pred_slots.clone()`` (MLPPatchDecoder + CNN image head, eval BatchNorm) -> nn.MSELoss on images + nn.MSELoss on slots
(weights 1 / 1, CONFIG.py:42-51) -> backward() through torch.autograd, decoder frozen, dropout inactive.
224 x 224, 7 slots, B = 2, 1 seed + 2 preds, ragged T5 masks.  Stored: both losses, the L2 norm of every parameter
gradient and four gradients (every 4th row / column of the large matrices).

Runs on the CPU in the build container, like make_golden.py:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_train_dino.py
"""

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

from make_golden import FixedNoise, build_reference_c4, c4_inputs  # noqa: E402
from textocvp_amd import synth  # noqa: E402

KS, B, P, SEED = 7, 2, 2, 91
KEEP = ("predictor.mlp_out.weight", "predictor.pe.pe", "predictor.predictor.0.attn.q.weight", "predictor.mlp_in.weight")


def train_dino_fixtures(out_dir):
    model, wrapper = build_reference_c4(num_slots=KS, num_context=1, num_preds=P)
    wrapper.eval()
    for p_ in model.parameters():
        p_.requires_grad_(False)
    videos, ids, mask = c4_inputs(B, 1 + P, 224, SEED)
    noise = synth.synth_noise(B, KS, 128, seed=SEED + 1)
    C, H, W = videos.shape[2:]
    with torch.no_grad(), FixedNoise(noise):
        hist = model(mode="decomp", x=videos, num_imgs=1 + P, decode=False, caption_tokens=ids,
                     attn_masks=mask)["slot_history"]
    pred_slots = wrapper(hist, caption_tokens=ids, attn_masks=mask)
    dec = model(mode="decode", slots=pred_slots.clone().reshape(B * P, KS, 128))
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
    np.savez(os.path.join(out_dir, "train_dino.npz"), loss_img=l_img.item(), loss_slot=l_slot.item(),
             names=np.array(names), grad_norms=np.array(norms, dtype=np.float64), ids=ids.numpy(),
             mask=mask.numpy(), pred_slots=pred_slots.detach().numpy(), **full)
    print("train_dino: losses", l_img.item(), l_slot.item(), "params", len(names), "kept", sorted(full))


if __name__ == "__main__":
    train_dino_fixtures(HERE)
