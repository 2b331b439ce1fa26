"""
SAVi configurations beyond the shipped SAVi.json (kernel 3 / 7, nearest x2 upsampling, eval batch-norm, 32 / 64 / 128
channel widths) on the CPU: checkpoint layout against manifests written from the reference
(tests/golden/make_golden_savi_variants.py), the phase-weight algebra of the fused upsampling in fp64, and the options
that stay refused.
"""

import copy
import json
import os

import pytest
import torch
import torch.nn.functional as F

from textocvp_amd import kernels as K
from textocvp_amd.setup_model import setup_model

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VARIANTS = ("up2", "k3", "bn_up2_128", "k7_mixed")


def manifest(tag):
    with open(os.path.join(GOLDEN, f"state_dict_manifest_savi_{tag}.json")) as f:
        return json.load(f)


def build(model_params):
    return setup_model({"model_name": "SAVi", "model_params": copy.deepcopy(model_params)}).eval()


@pytest.mark.parametrize("tag", VARIANTS)
def test_variant_state_dict_matches_reference_manifest(tag):
    man = manifest(tag)
    savi = build(man["model_params"])
    sd = savi.state_dict()
    assert {k: list(v.shape) for k, v in sd.items()} == man["SAVi"]
    # a reference-layout checkpoint loads strictly
    ckpt = {k: torch.zeros(s, dtype=sd[k].dtype) for k, s in man["SAVi"].items()}
    savi.load_state_dict(ckpt, strict=True)


def test_upsampling_decoder_keys_sit_at_the_reference_indices():
    man = manifest("up2")
    dec = sorted({k.split(".")[2] for k in man["SAVi"] if k.startswith("decoder.decoder.")})
    assert dec == ["0", "2", "4", "6", "7"]
    bn = manifest("bn_up2_128")["SAVi"]
    for leaf in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked"):
        assert f"decoder.decoder.2.block.1.{leaf}" in bn


def _phase_conv(x, wph, k):
    """ "nearest x2 -> k x k conv" evaluated as four phase convolutions over the source image (fp64) """
    n, cin, SH, SW = x.shape
    T = k // 2 + 1
    cout = wph.shape[2]
    y = torch.zeros((n, cout, 2 * SH, 2 * SW), dtype=torch.float64)
    for a in range(2):
        oa = (a - k // 2) // 2
        for b in range(2):
            ob = (b - k // 2) // 2
            w = wph[2 * a + b].reshape(T, T, cout, cin).permute(2, 3, 0, 1)
            xp = F.pad(x, (-ob, ob + T - 1, -oa, oa + T - 1))
            y[:, :, a::2, b::2] = F.conv2d(xp, w)
    return y


@pytest.mark.parametrize("k", [3, 5, 7])
def test_phase_weights_reproduce_upsampled_conv_in_fp64(k):
    g = torch.Generator().manual_seed(k)
    w = torch.randn((6, 5, k, k), generator=g, dtype=torch.float64)
    x = torch.randn((2, 5, 9, 7), generator=g, dtype=torch.float64)
    ref = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, padding=k // 2)
    # packing in fp64, the kernels round the packed sums once to fp32
    wph = K.pack_conv_up2_weights(w).double()
    assert wph.shape == (4, (k // 2 + 1) ** 2, 6, 5)
    got = _phase_conv(x, wph, k)
    assert (got - ref).abs().max().item() <= 1e-6 * ref.abs().max().item()
    # exact when the weight sums are representable (integer weights)
    wi = torch.randint(-8, 8, (6, 5, k, k), generator=g).double()
    ref_i = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), wi, padding=k // 2)
    assert torch.allclose(_phase_conv(x, K.pack_conv_up2_weights(wi).double(), k), ref_i, rtol=0, atol=1e-12)


def test_phase_weights_of_kernel3_match_the_image_head_packing():
    w = torch.randn((8, 4, 3, 3))
    assert torch.equal(K.pack_conv_up2_weights(w), K.pack_conv3x3_up2_weights(w))


def _cfg(**dec):
    p = copy.deepcopy(manifest("up2")["model_params"])
    p["decoder"]["decoder_params"].update(dec)
    return p


@pytest.mark.parametrize("edit", [dict(upsample=3), dict(upsample=4), dict(stride=2), dict(kernel_size=9),
                                  dict(kernel_size=3, num_channels=[48, 64, 64, 64]),
                                  dict(num_channels=[64, 64, 96, 64])])
def test_unsupported_decoder_options_still_raise(edit):
    with pytest.raises(NotImplementedError):
        build(_cfg(**edit))


@pytest.mark.parametrize("edit", [dict(batch_norm=True), dict(stride=2), dict(kernel_size=3, num_channels=[32, 48, 32, 32]),
                                  dict(kernel_size=9), dict(downsample_encoder=True)])
def test_unsupported_encoder_options_still_raise(edit):
    from textocvp_amd.models.EncodersDecoders.encoders import SimpleConvEncoder
    params = dict(hidden_dims=[32, 32, 32, 32], kernel_size=5)
    if "num_channels" in edit:
        params["hidden_dims"] = edit.pop("num_channels")
    params.update(edit)
    with pytest.raises(NotImplementedError):
        SimpleConvEncoder(in_channels=3, **params)


def test_upsample_marker_refuses_other_factors():
    from textocvp_amd.models.Blocks.model_blocks import Upsample
    assert repr(Upsample(2)) == "Upsample(scale_factor=2)"
    with pytest.raises(NotImplementedError):
        Upsample(3)


@pytest.mark.parametrize("tag", VARIANTS)
def test_decoder_training_refuses_variants(tag):
    from textocvp_amd.train.decoder import DecoderLoss
    savi = build(manifest(tag)["model_params"])
    if not savi.decoder.generic:
        pytest.fail("every variant takes the generic decoder path")
    with pytest.raises(NotImplementedError, match="kernel_size|upsample|batch_norm"):
        DecoderLoss(savi)


def test_shipped_config_keeps_its_decoder_path():
    from textocvp_amd.setup_model import default_exp_params
    savi = setup_model(default_exp_params(num_slots=7)["model"])
    assert not savi.decoder.generic and savi.decoder.upsample is None
    assert savi.decoder.output_size((64, 64)) == (64, 64)
    up2 = build(manifest("up2")["model_params"])
    assert up2.decoder.output_size((8, 8)) == (64, 64)
