"""Host side of the 8-bit blockwise AdamW (csrc/optim8.hip; the reference's ``--use_8bit_adam`` = ``bitsandbytes.optim.AdamW8bit``,
diffusion/train_controlnet_genima.py:224, :1163-1175; Dettmers et al., "8-bit Optimizers via Block-wise Quantization"):
the two 256-entry dynamic code maps and the table of quantisation blocks over a ``TrainParams.layout``.

The moments of a parameter with at least ``MIN_8BIT_SIZE`` elements are stored as one code byte per element plus one f32 ``absmax`` per
block of ``BLOCK`` consecutive elements; value = map[code] * absmax.  The first moment uses the signed map, the second the unsigned one.
Smaller parameters (biases, norm weights) keep fp32 moments (bitsandbytes' ``min_8bit_size``).
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import torch

BLOCK = 256           # elements per quantisation block (one wave of the kernel: 64 lanes x 4 elements)
MIN_8BIT_SIZE = 4096  # parameters with fewer elements keep fp32 moments
KIND = "adamw8bit"    # the checkpoint marker of this optimizer's state ("adamw" = two flat fp32 moment buffers)


def dynamic_map(signed: bool, max_exponent_bits: int = 7, total_bits: int = 8) -> torch.Tensor:
    """The "dynamic tree" code map: f32 [2 ** total_bits], sorted.  Exponent i of ``max_exponent_bits`` decades (10 ** (i - 6)) carries the
    midpoints of 2 ** i (signed; both signs) or 2 ** (i + 1) (unsigned) equal steps over [0.1, 1]; 0 and 1 complete the map.
    Signed: 127 positive + 127 negative + {0, 1}, range [-0.993, 1]; unsigned: 254 positive + {0, 1}, range [0, 1]."""
    non_sign_bits = total_bits - 1
    data: List[float] = []
    for i in range(max_exponent_bits):
        items = 2 ** (i + non_sign_bits - max_exponent_bits) + 1 if signed else 2 ** (i + non_sign_bits - max_exponent_bits + 1) + 1
        edges = torch.linspace(0.1, 1.0, items, dtype=torch.float32)
        means = (edges[:-1] + edges[1:]) / 2.0
        scale = 10.0 ** (-(max_exponent_bits - 1) + i)
        data += (scale * means).tolist()
        if signed:
            data += (-scale * means).tolist()
    data += [0.0, 1.0]
    assert len(data) == 2 ** total_bits, len(data)
    return torch.tensor(sorted(data), dtype=torch.float32)


def _numel(shape: Sequence[int]) -> int:
    n = 1
    for s in shape:
        n *= s
    return n


def build_block_table(layout) -> Tuple[torch.Tensor, List[Tuple[int, int]], int, int]:
    """``layout``: name -> (offset, shape) of a flat parameter buffer (TrainParams.layout; offsets are multiples of 8, untouched here).
    -> (table, small_ranges, n8, n_small):

    * ``table`` int64 [n_blocks, 2]: (element offset in the flat buffer, code offset * 512 + length).  Blocks tile every parameter with
      >= MIN_8BIT_SIZE elements in runs of BLOCK; none crosses a parameter boundary (a tensor never inherits its neighbour's absmax) and
      the last block of a parameter may be short.  Code offsets are the running sum of the lengths: the code buffers hold ``n8`` bytes.
      The kernel moves a lane's four codes as one dword only where the code offset is a multiple of 4, so a quantised parameter whose
      element count is not would send every later block down the byte-wise path (correct, slower).  Every packed layout of this
      project has counts that are multiples of 8 (tests/test_adamw8_cpu.py checks the tiny and the SD-Turbo ControlNet).
    * ``small_ranges``: (start, end) element ranges of the flat buffer covering the smaller parameters, adjacent ones merged; they sum
      to ``n_small`` elements and keep fp32 moments in compact buffers of that size, in this order."""
    rows: List[Tuple[int, int]] = []
    small: List[Tuple[int, int]] = []
    n8 = n_small = 0
    for _, (off, shape) in layout.items():
        n = _numel(shape)
        if n < MIN_8BIT_SIZE:
            if small and small[-1][1] == off:
                small[-1] = (small[-1][0], off + n)
            else:
                small.append((off, off + n))
            n_small += n
            continue
        for b in range(0, n, BLOCK):
            ln = min(BLOCK, n - b)
            rows.append((off + b, ((n8 + b) << 9) | ln))
        n8 += n
    table = torch.tensor(rows, dtype=torch.int64).reshape(-1, 2)
    return table, small, n8, n_small


def table_blocks(table: torch.Tensor) -> List[Tuple[int, int, int]]:
    """The table decoded: [(element offset, code offset, length)]."""
    return [(int(o), int(w) >> 9, int(w) & 511) for o, w in table.tolist()]
