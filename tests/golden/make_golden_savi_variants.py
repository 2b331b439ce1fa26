"""
Golden vectors of SAVi configurations other than the shipped SAVi.json, produced by the reference's own SAVi built from
edited SAVi.json dicts (eval mode, synthetic weights of synth.fill_module_, BatchNorm running statistics of
synth.fill_batchnorm_stats_):

    tag          video     encoder                      decoder
    up2          64x64     as shipped                   k 5, resolution 8x8, upsample 2, 4 x 64
    k3           64x64     k 3                          k 3, no upsampling
    bn_up2_128   128x128   as shipped (resolution 128)  k 5, batch_norm, resolution 16x16, upsample 2
    k7_mixed     64x64     k 7, [32, 64, 64, 64]        k 7, num_channels [32, 64, 64, 128]

Per variant: savi_<tag>.npz (encoder features of two synthetic images at every feat_step-th position; decode of fixed
slots: recons_imgs every img_step-th pixel, recons / masks every sub_step-th, slot-index maps in full; for up2 and
bn_up2_128 a forward_eval with TextOCVP_CustomTF, K = 7, B = 1, 1 seed + 2 preds, predicted images every img_step-th
pixel; the 128 x 128 variant is sub-sampled more so that every file stays small) and
state_dict_manifest_savi_<tag>.json (the model_params the SAVi was built from and its state_dict keys / shapes).  Runs on the CPU, like make_golden.py:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_savi_variants.py [out_dir]
"""

import copy
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

from make_golden import forward_eval, import_reference, load_cfg  # noqa: E402
from textocvp_amd import synth  # noqa: E402

KS, D, SEED = 7, 128, 0


def variant_cfg(tag):
    """ SAVi.json with the variant's edits """
    cfg = load_cfg("models/SAVi.json")
    cfg["num_slots"] = KS
    enc, dec = cfg["encoder"]["encoder_params"], cfg["decoder"]["decoder_params"]
    if tag == "up2":
        dec.update(resolution=[8, 8], upsample=2)
    elif tag == "k3":
        enc.update(kernel_size=3)
        dec.update(kernel_size=3)
    elif tag == "bn_up2_128":
        enc.update(resolution=[128, 128])
        dec.update(batch_norm=True, resolution=[16, 16], upsample=2)
    elif tag == "k7_mixed":
        enc.update(kernel_size=7, num_channels=[32, 64, 64, 64])
        dec.update(kernel_size=7, num_channels=[32, 64, 64, 128])
    else:
        raise ValueError(tag)
    return cfg


VARIANTS = ("up2", "k3", "bn_up2_128", "k7_mixed")
E2E = ("up2", "bn_up2_128")


def image_size(cfg):
    return tuple(cfg["encoder"]["encoder_params"]["resolution"])


def build_variant(tag, num_context=1, num_preds=2):
    """ the reference's SAVi (+ PredictorWrapper(TextOCVP_CustomTF)) for a variant, synthetic weights, eval mode """
    SAVi, TextOCVP_CustomTF, PredictorWrapper = import_reference()
    cfg = variant_cfg(tag)
    savi = SAVi(**copy.deepcopy(cfg)).eval()
    synth.fill_module_(savi, seed=SEED, prefix="savi.")
    synth.fill_batchnorm_stats_(savi, seed=SEED, prefix="savi.")
    pred_cfg = load_cfg("predictors/TextOCVP_CustomTF.json")
    pp = copy.deepcopy(pred_cfg["predictor_params"])
    pp["predictor_params"]["input_buffer_size"] = 10
    core = TextOCVP_CustomTF(slot_dim=cfg["slot_dim"], predictor_params=pp["predictor_params"],
                             fusion_params=pp["fusion_params"], text_encoder_params=pp["text_encoder_params"])
    exp_params = {
        "model": {"model_name": "SAVi", "model_params": copy.deepcopy(cfg)},
        "predictor": copy.deepcopy(pred_cfg),
        "prediction_params": {"num_context": num_context, "num_preds": num_preds, "teacher_force": False,
                              "input_buffer_size": 10},
    }
    wrapper = PredictorWrapper(exp_params=exp_params, predictor=core).eval()
    synth.fill_module_(wrapper, seed=SEED, prefix="pred.")
    pe = wrapper.predictor.pe.pe
    with torch.no_grad():
        pe.copy_(synth.synth_tensor("pred.predictor.pe.pe", pe.shape, "normal", pe.shape[-1] ** -0.5, SEED))
    return cfg, savi, wrapper


@torch.no_grad()
def variant_fixtures(tag, out_dir):
    cfg, savi, wrapper = build_variant(tag)
    H, W = image_size(cfg)
    step, feat_step, img_step = (4, 16, 1) if H <= 64 else (8, 64, 2)
    fx = {}
    imgs = synth.synth_tensor(f"variants.{tag}.imgs", (2, 3, H, W), "unit")
    fx["encoder_feats_sub"] = savi.encode(imgs)[:, ::feat_step].numpy()
    dslots = synth.synth_tensor(f"variants.{tag}.dec_slots", (2, KS, D), "normal")
    out = savi(mode="decode", slots=dslots)
    fx["dec_recons_imgs_sub"] = out["recons_imgs"][..., ::img_step, ::img_step].numpy()
    fx["dec_recons_sub"] = out["recons"][..., ::step, ::step].numpy()
    fx["dec_masks_sub"] = out["masks"][..., ::step, ::step].numpy()
    fx["dec_masks_argmax"] = out["masks"].argmax(dim=1).to(torch.uint8).numpy()
    fx.update(sub_step=np.int64(step), feat_step=np.int64(feat_step), img_step=np.int64(img_step))
    if tag in E2E:
        videos = synth.synth_videos(1, 3, height=H, width=W, seed=SEED)
        tokens, lengths = synth.synth_captions(1, max_len=10, seed=SEED)
        noise = synth.synth_noise(1, KS, D, seed=SEED + 1)
        sh, ps, pi, od = forward_eval(savi, wrapper, videos, tokens, lengths, noise, 1, 2)
        fx.update(e2e_slot_history=sh.numpy(), e2e_pred_slots=ps.numpy(),
                  e2e_pred_imgs_sub=pi[..., ::img_step, ::img_step].numpy(),
                  e2e_masks_argmax=od["masks"].argmax(dim=1).to(torch.uint8).numpy())
    np.savez_compressed(os.path.join(out_dir, f"savi_{tag}.npz"), **fx)
    man = {"model_params": cfg, "SAVi": {k: list(v.shape) for k, v in savi.state_dict().items()}}
    with open(os.path.join(out_dir, f"state_dict_manifest_savi_{tag}.json"), "w") as f:
        json.dump(man, f, indent=0, sort_keys=True)
    print(f"savi_{tag}:", {k: getattr(v, "shape", v) for k, v in fx.items()})


if __name__ == "__main__":
    torch.set_num_threads(8)
    out = sys.argv[1] if len(sys.argv) > 1 else HERE
    for tag in VARIANTS:
        variant_fixtures(tag, out)
