"""-m gpu: ``attach_frozen(..., augmentations=)`` with blur and affine inside ``train_step`` on the tiny families, for the ControlNet
trainer and the InstructPix2Pix trainer.  Run A augments inside the step; run B applies ``augment_data`` beforehand with a generator
seeded like A's ``_gen_cpu``, hands that generator's state on and steps without augmentation: the two losses are bit-identical, so
the step augments first, with the trainer's generator, in the reference's roles.  For InstructPix2Pix the loss must also differ from
the unaugmented step's (the option was silently dropped before)."""
import pytest
import torch

from genima_amd import augment, configs, schema, weights
from genima_amd.engine import Engine
from genima_amd.packing import pack_state_dict
from genima_amd.pix2pix import InstructPix2PixTrainer, expand_conv_in
from genima_amd.scheduler import DDPMScheduler
from genima_amd.training import ControlNetTrainer
from util import q16

pytestmark = pytest.mark.gpu
AUGS = "crop,colorjitter,blur,affine"
SEED = 5


def _synth(sch, s):
    return weights.round_to(weights.synth_state_dict(sch, s), torch.float16)


def _controlnet(E, augmentations):
    fam = configs.family("tiny")
    tr = ControlNetTrainer(E, fam["unet"], fam["controlnet"], pack_state_dict(_synth(schema.unet_schema(fam["unet"]), 1), "cuda"),
                           _synth(schema.controlnet_schema(fam["controlnet"]), 2), lr=1e-4, loss_scale=4096.0)
    tr.attach_frozen(fam["vae"], pack_state_dict(_synth(schema.vae_schema(fam["vae"]), 3), "cuda"), fam["text"],
                     pack_state_dict(_synth(schema.clip_text_schema(fam["text"]), 4), "cuda"), DDPMScheduler(), seed=SEED,
                     augmentations=augmentations)
    return tr


def _pix2pix(E, augmentations):
    fam = configs.family("tiny-pix2pix")
    usd = weights.round_to(expand_conv_in(weights.synth_state_dict(schema.unet_schema(dict(fam["unet"], in_channels=4)), 1), 8), torch.float16)
    tr = InstructPix2PixTrainer(E, fam["unet"], usd, lr=1e-4, loss_scale=4096.0)
    tr.attach_frozen(fam["vae"], pack_state_dict(_synth(schema.vae_schema(fam["vae"]), 3), "cuda"), fam["text"],
                     pack_state_dict(_synth(schema.clip_text_schema(fam["text"]), 4), "cuda"), DDPMScheduler(), seed=SEED,
                     augmentations=augmentations)
    return tr


def _pre_augmented_loss(E, make, batch, roles):
    """Run B: augment_data outside the step with a generator seeded like _gen_cpu, then a step without augmentation."""
    tr = make(E, None)
    g = torch.Generator().manual_seed(SEED)
    dev = {k: tr._nhwc8(batch[k]) for k in roles}
    aug = augment.augment_data(E, AUGS, dev, g, roles=roles)
    tr._gen_cpu.set_state(g.get_state())
    return float(tr.train_step(dict(batch, **{k: aug[k] for k in roles})))


def test_controlnet_step_augments_with_blur_and_affine():
    E = Engine("cuda:0")
    B, R = 2, 256
    g = torch.Generator().manual_seed(9)
    batch = dict(pixel_values=q16(torch.rand(B, 3, R, R, generator=g) * 2 - 1), conditioning_pixel_values=q16(torch.rand(B, 3, R, R, generator=g)),
                 input_ids=torch.randint(0, 1000, (B, 77), generator=g))
    a = _controlnet(E, AUGS)
    loss_a = float(a.train_step(batch))
    loss_b = _pre_augmented_loss(E, _controlnet, batch, augment.ROLES)
    print(f"ControlNet step with {AUGS}: {loss_a!r} (in the step) vs {loss_b!r} (augmented beforehand)")
    assert loss_a == loss_b and loss_a == loss_a


def test_pix2pix_step_augments_instead_of_dropping_the_option():
    E = Engine("cuda:0")
    B, R = 2, 256
    g = torch.Generator().manual_seed(3)
    batch = dict(original_pixel_values=q16(torch.rand(B, 3, R, R, generator=g) * 2 - 1),
                 edited_pixel_values=q16(torch.rand(B, 3, R, R, generator=g) * 2 - 1), input_ids=torch.randint(0, 1000, (B, 77), generator=g))
    a = _pix2pix(E, AUGS)
    loss_a = float(a.train_step(batch))
    loss_b = _pre_augmented_loss(E, _pix2pix, batch, augment.P2P_ROLES)
    loss_c = float(_pix2pix(E, None).train_step(batch))
    print(f"pix2pix step with {AUGS}: {loss_a!r} (in the step) vs {loss_b!r} (augmented beforehand); without augmentation {loss_c!r}")
    assert loss_a == loss_b and loss_a == loss_a
    assert loss_c != loss_a
