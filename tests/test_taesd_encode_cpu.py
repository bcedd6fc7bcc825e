"""-m "not gpu": the TAESD encoder's ABI (gn_tiny_block, csrc/taesd.hip) and the fp32 restatement of diffusers 0.29 ``EncoderTiny`` /
``AutoencoderTinyBlock`` that the GPU tests (test_taesd_encode_gpu.py) hold the device encoder to."""
import os
import re

import torch
import torch.nn.functional as F

from genima_amd import _lib, configs, schema, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tiny_block_ref(x, sd, p, q=lambda t: t):
    """AutoencoderTinyBlock with the identity skip: relu(conv(relu(conv(relu(conv(x))))) + x), NCHW.  ``q``: storage rounding of each
    intermediate (identity = fp32)."""
    h = q(F.relu(F.conv2d(x, sd[p + ".conv.0.weight"], sd[p + ".conv.0.bias"], padding=1)))
    h = q(F.relu(F.conv2d(h, sd[p + ".conv.2.weight"], sd[p + ".conv.2.bias"], padding=1)))
    return q(F.relu(F.conv2d(h, sd[p + ".conv.4.weight"], sd[p + ".conv.4.bias"], padding=1) + x))


def encoder_tiny_ref(x, sd, cfg, q=lambda t: t):
    """EncoderTiny.forward: layers(x.add(1).div(2)) -- conv_in, per stage (a stride-2 bias-free conv from stage 2 on, blocks), conv_out."""
    h = q(q(x + 1) / 2)
    idx = 0
    for i, n in enumerate(cfg["num_encoder_blocks"]):
        p = f"encoder.layers.{idx}"
        h = q(F.conv2d(h, sd[p + ".weight"], sd.get(p + ".bias"), stride=1 if i == 0 else 2, padding=1))
        idx += 1
        for _ in range(n):
            h = tiny_block_ref(h, sd, f"encoder.layers.{idx}", q)
            idx += 1
    p = f"encoder.layers.{idx}"
    return q(F.conv2d(h, sd[p + ".weight"], sd[p + ".bias"], padding=1))


class _Reads(dict):
    """state dict that records the keys read"""

    def __init__(self, sd):
        super().__init__(sd)
        self.read = set()

    def __getitem__(self, k):
        self.read.add(k)
        return super().__getitem__(k)

    def get(self, k, default=None):
        if k in self:
            self.read.add(k)
        return super().get(k, default)


def test_tiny_block_abi_declared_and_bound():
    src = open(os.path.join(ROOT, "include", "genima_hip.h")).read()
    for name in ("gn_tiny_block", "gn_tiny_block_supported", "gn_program_add_tiny_block"):
        assert re.search(r"\b" + name + r"\s*\(", src), f"{name} is not declared in include/genima_hip.h"
        assert name in _lib.SIGNATURES, f"{name} is not bound in _lib.SIGNATURES"
    assert _lib.ABI_VERSION == 101


def test_restatement_shape_and_parameter_count():
    cfg = configs.TAESD
    sch = schema.taesd_schema(cfg, decoder=False)
    sd = _Reads(weights.round_to(weights.synth_state_dict(sch, 3), torch.float16))
    B, H, W = 2, 64, 48
    x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(0)) * 2 - 1
    with torch.no_grad():
        y = encoder_tiny_ref(x, sd, cfg)
    assert tuple(y.shape) == (B, cfg["latent_channels"], H // 8, W // 8)
    assert torch.isfinite(y).all()
    # the restatement reads every encoder parameter of the schema, and nothing else
    assert sd.read == set(sch)
    assert sum(sd[k].numel() for k in sd.read) == schema.param_count(sch) == 1_222_532
