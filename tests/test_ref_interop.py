"""Checkpoint interoperability proof vs the reference implementation.

For one model per flagship family: a digest of the reference model's state-dict
layout (every key with its shape) and its logits were recorded in
tests/golden/ref_interop.json (by tools/gen_ref_interop_golden.py, which loads
our seeded random-init state dict into the reference model by exact key match).
The test rebuilds the same seeded model and input and asserts identical key
sets and tensor shapes (equal digests), and logits that agree.  This is the strongest possible "timm checkpoint format"
guarantee available offline (no network for real pretrained weights): identical
layouts and identical math given identical weights.
"""
import hashlib
import json
import os

import pytest
import torch

import timm_amd

GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_interop.json')


def layout_digest(state_dict):
    """sha256 over the sorted 'key shape' lines: equal iff key sets and shapes are."""
    lines = sorted(f'{k} {tuple(v.shape)}' for k, v in state_dict.items())
    return hashlib.sha256('\n'.join(lines).encode()).hexdigest()


@pytest.fixture(scope='module')
def goldens():
    with open(GOLDEN_FILE) as f:
        return json.load(f)


def seeded_model_and_input(model_name, img_size, input_scale=1.0):
    """The model and input both the golden generator and the test build.

    A few nets without normalisation at init (eval-mode BN with fresh running
    stats) blow a unit-variance input up to logits of 1e2..1e15, where an
    absolute 1e-4 bound only holds for bit-identical arithmetic.  The generator
    records a power-of-ten input_scale for those so the recorded logits are
    O(1) and the bound means the same on every host.
    """
    torch.manual_seed(42)
    model = timm_amd.create_model(model_name, num_classes=10)
    model.eval()
    x = torch.randn(2, 3, img_size, img_size) * input_scale
    return model, x


# (model, input size) — small/flagship variant per family
INTEROP_MODELS = [
    ('vit_tiny_patch16_224', 224),
    ('vit_base_patch16_224', 224),
    ('deit_tiny_distilled_patch16_224', 224),
    ('eva02_tiny_patch14_224', 224),
    ('beit_base_patch16_224', 224),
    ('convnext_atto', 128),
    ('convnextv2_atto', 128),
    ('swin_tiny_patch4_window7_224', 224),
    ('swinv2_tiny_window8_256', 256),
    ('aimv2_large_patch14_224', 224),
    ('flexivit_small', 240),
    ('beit3_base_patch16_224', 224),
    ('test_vit3', 160),
    ('mobilenetv3_small_050', 128),
    ('coatnet_nano_rw_224', 224),
    ('coatnet_0_rw_224', 224),
    ('maxvit_rmlp_nano_rw_256', 256),
    ('maxvit_tiny_pm_256', 256),
    ('coatnext_nano_rw_224', 224),
    ('maxxvitv2_nano_rw_256', 256),
    ('mobileone_s0', 128),
    ('regnetz_005', 128),
    ('regnetz_b16', 128),
    ('resnet50_clip_gap', 224),
    ('nf_regnet_b0', 128),
    ('efficientnet_b0', 128),
    ('mobilenetv3_small_100', 128),
    ('mobilenetv4_conv_small', 128),
    ('resnet18', 128),
    ('resnet50', 128),
    ('resnetv2_50', 128),
    ('regnety_002', 128),
    ('hiera_tiny_224', 224),
    ('mixer_s16_224', 224),
    ('vgg11', 128),
    ('densenet121', 128),
    ('nfnet_l0', 224),
    ('ghostnet_100', 128),
    ('repvgg_a0', 128),
    ('xcit_nano_12_p16_224', 224),
    ('pvt_v2_b0', 128),
    ('coat_tiny', 224),
    ('levit_128s', 224),
    ('efficientformer_l1', 224),
    ('poolformer_s12', 128),
    ('gcvit_xxtiny', 224),
    ('focalnet_tiny_srf', 128),
    ('edgenext_xx_small', 128),
    ('cait_xxs24_224', 224),
    ('convmixer_768_32', 224),
    ('dpn68', 128),
    ('hardcorenas_a', 128),
]


@pytest.mark.parametrize('model_name,img_size', INTEROP_MODELS)
def test_state_dict_and_logit_interop(goldens, model_name, img_size):
    if not timm_amd.is_model(model_name):
        pytest.fail(f'{model_name} missing from timm_amd registry')
    golden = goldens[model_name]
    assert golden['img_size'] == img_size

    our_model, x = seeded_model_and_input(model_name, img_size, golden['input_scale'])

    # key sets and shapes: the generator prints the differing keys when this trips
    our_sd = our_model.state_dict()
    assert len(our_sd) == golden['num_keys'], \
        f'state dict keys differ: ours {len(our_sd)} reference {golden["num_keys"]}'
    assert layout_digest(our_sd) == golden['layout_sha256'], \
        'state dict keys or shapes differ from the reference layout'

    ref_out = torch.tensor(golden['logits'], dtype=torch.float32)
    with torch.no_grad():
        our_out = our_model(x)
    if isinstance(our_out, (tuple, list)):
        our_out = our_out[0]
    assert our_out.shape == ref_out.shape
    err = (ref_out.float() - our_out.float()).abs().max().item()
    assert err < 1e-4, f'logit mismatch {err}'
