"""cvd3_kernel (cvp.hip): the stride-2 data gradients whose weights stream through an LDS-DMA ring behind counted waits.

Exact operands (tools/exact_operands.py; every stored value equal to the fp64 reference bit for bit) on the smallest shapes that
reach every path of the ring, in the tuple convention of exact_operands.BACKWARD (B, H, W, Cin, Cout, R, S, pad, transposed, mode),
each with and without the accumulated old gradient (which the epilogue prefetches):
  head form (mode 1, 128 -> 64): 16 chunk pairs in one channel group - 32 chunks, the ring of 4 wraps 8 times
    3 x 17 x 33: 27 tiles, partial in both directions, more than one tile per XCD range
    1 x 8 x 16:  exactly one full tile
  ConvTranspose form (nine taps, 1 + 2 + 2 + 4 per class, Cout / 64 channel groups)
    128 -> 128 at 2 x 9 x 17: two groups, 18 stages (not a multiple of the ring depth), groups of 2, 4, 4 and 8 chunks
    384 -> 256 at 1 x 5 x 3: four groups, three column tiles (ntn = 3)
    256 -> 384 at 1 x 5 x 3: six groups, two column tiles (ntn = 2)
One filled-chip case per form: a refill that overtakes a fragment read of the slot it rewrites is a matter of timing (conv3.hip's
K loop records one that showed at production size only).  Each runs twice; both runs must be exact, hence identical.  A failure
there is a finding about the ring's waits: read them (the counted barriers of the walk), do not loop the case."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DT = [1, 2]
DT_IDS = ["fp16", "bf16"]

#        name                      B   H    W   Cin  Cout R  S pad T mode
SMALL = [
    ("head 3x17x33",               3, 17,  33, 128,  64, 3, 3, 1, 0, 1),
    ("head 1x8x16",                1,  8,  16, 128,  64, 3, 3, 1, 0, 1),
    ("convT 128->128 2x9x17",      2,  9,  17, 128, 128, 3, 3, 1, 1, 0),
    ("convT 384->256 1x5x3",       1,  5,   3, 384, 256, 3, 3, 1, 1, 0),
    ("convT 256->384 1x5x3",       1,  5,   3, 256, 384, 3, 3, 1, 1, 0),
]
FILLED = [
    ("head 4x160x240",             4, 160, 240, 128,  64, 3, 3, 1, 0, 1),
    ("convT 256->256 4x80x120",    4,  80, 120, 256, 256, 3, 3, 1, 1, 0),
]


@pytest.fixture(scope="module")
def lab():
    assert torch.cuda.is_available()
    from tools import gpu_lab
    return gpu_lab


def _run(lab, c, dtype, acc):
    name, B, H, W, Cin, Cout, R, S, pad, transposed, mode = c
    return lab.backward_case(name, dtype, B, H, W, Cin, Cout, R, S, pad, transposed=transposed, with_q=0, acc=acc, what="dgrad",
                             mode=mode, expect="cvp", exact=True)


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("acc", [0, 1], ids=["store", "accumulate"])
@pytest.mark.parametrize("case", range(len(SMALL)), ids=[c[0].replace(" ", "_") for c in SMALL])
def test_ring_walk_is_exact(lab, case, acc, dtype):
    assert _run(lab, SMALL[case], dtype, acc)


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("case", range(len(FILLED)), ids=[c[0].replace(" ", "_") for c in FILLED])
def test_ring_on_a_filled_chip_is_exact_twice(lab, case, dtype):
    c = FILLED[case]
    name, B, H, W, Cin, Cout = c[:6]
    tiles = B * ((H + 7) // 8) * ((W + 15) // 16) * (Cin // 128)
    assert tiles >= 2 * 256, "fewer than two workgroups per compute unit"
    assert _run(lab, c, dtype, 1)
    assert _run(lab, c, dtype, 1)
