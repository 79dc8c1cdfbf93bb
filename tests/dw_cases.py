"""The depthwise parity cases, one row per launch, each naming the kernel family it is FOR (csrc/dwconv_route.h).

A parity test that picks a shape and trusts the dispatcher to reach the kernel its author had in mind checks another kernel
as soon as one argument changes the route.  Here the family is part of the row: test_dw_route.py asks the pure route function
(no GPU) that every row reaches the family it names and that every (direction, family, k, stride, dtype) cell a family's `can`
accepts keeps its rows; test_gpu_dwconv.py asserts the route again in front of every launch.

Row: direction ('fwd' | 'bwd'), family (T3D_DW_* without the prefix), dtype, B, C, H, W, k, stride,
     pooled  forward: pooled sums (gap_sum) are requested,
     gated   forward: a squeeze-excite gate in the prologue (mode se_pre / se_post),
     forced  the automatic route gives this call to ANOTHER family: the row runs under t3d_dwconv_force_route(family),
     mode    forward: plain | bnact-<act> | se_pre | se_post;  backward: plain_res | bnact | bnact_ps | bnact-<act>,
     stats   forward: BatchNorm statistics are requested (False: stats = NULL, and these rows have pooled = 0 as well).
This module is data: no torch, no native library."""
import itertools
from collections import namedtuple

Case = namedtuple('Case', 'direction family dtype B C H W k stride pooled gated forced mode stats')

TRAIN, ALL = ('f32', 'bf16'), ('f32', 'bf16', 'f16')

# ---- shapes (B, C, H, W), each there for a boundary of some launcher ---------------------------------------------------
P1 = (1, 8, 1, 1)         # 3x3: eight of nine taps are padding
P2 = (1, 24, 2, 2)
ODD = (3, 40, 13, 17)     # flattened (column, channel group) mapping; odd Wo: half of the last column pair is empty
SLAB8 = (5, 264, 9, 7)    # channel slabs (C >= 256) with an 8-channel last slab
SLAB2 = (2, 512, 4, 3)    # exactly two full slabs
CHUNK = (2, 16, 37, 5)    # 37 (stride 2: 19) rows in chunks that do not divide them: 4 x 10, 2 x 10, 7 x 6, 4 x 5 -- every row walk
EVEN = (2, 32, 5, 6)      # even W above 2: the second column of the last pair has its right tap outside the image
SLAB1 = (1, 256, 3, 4)    # the same in the slab mapping, exactly one slab
LOOP = (2100, 8, 2, 2)    # more work items than blocks: the persistent item / tile loops with their carried sums
# the same in the slab mapping: 3200 items for 3072 waves.  (Three rows, not one: in bf16 every wave's partial sum of squares is
# snapped onto the order-independent grid of csrc/common.h, 2^-17 here, so a channel needs all nine taps' worth of signal for
# 3072 snapped partials to stay inside the 1e-5 relative margin of the statistics check.)
LOOPS = (400, 256, 3, 16)
SLABP = (2, 496, 3, 5)    # a last slab with 60 of 64 lanes (forward), 56 of 64 (stride-1 backward: slabs only below 12 % idle lanes)
S3 = (P1, P2, ODD, SLAB8, SLAB2, CHUNK, EVEN, SLAB1, SLABP, LOOP, LOOPS)
S3_TILE = tuple(p for p in S3 if p[2] >= 2 and p[3] >= 2)      # the register tiles need a 2x2 plane
Q2 = (1, 8, 2, 2)         # 5x5: plane smaller than the kernel
Q3 = (4, 960, 3, 3)
T8 = (2, 24, 8, 8)        # lower bound of the 5x5 tiles
T913 = (2, 48, 9, 13)     # tiles hanging over both edges
P7 = (3, 72, 7, 7)        # plane kernel: partial 128-channel slab
P7B = (2, 136, 7, 7)      # plane kernel: a full slab and an 8-channel one
P7C = (5, 960, 7, 7)
TALL, WIDE = (1, 8, 65, 8), (1, 8, 8, 65)     # first planes the automatic route gives to the k x k walk at stride 1
TALL2 = (1, 8, 29, 8)                         # the same at stride 2
MID = (2, 72, 20, 20)     # 5x5 with real interior taps
LONG = (1, 16, 70, 9)     # tiles can, but are not wanted
TLOOP = (110, 8, 32, 35)  # 5x5 tiles: more tiles than waves in either direction and stride (4400 forward for 4096, 8800 backward for 2048)
P7L = (2100, 8, 7, 7)     # plane kernel: more planes than its 2048 waves
W6 = (2, 24, 9, 6)        # k x k walk, four columns per thread at stride 1: two of the last four are outside
KSLAB = (2, 248, 6, 6)    # k x k walk in slabs (124 channel pairs: under 8 % idle lanes), the last slab partial
KFLAT, KSLABS = (1, 296, 5, 6), (1, 304, 5, 6)     # 5x5 backward walk: the widest flattened block (its fp64 scratch just fits LDS), the first forced into slabs
LDSH = (1, 64, 9, 33)     # LDS tiles of 64 staged channels x 16 columns: the tile height is halved until they fit (5x5: down to one row)

FWD_MODES = (('plain', True), ('bnact-hswish', True), ('bnact-relu6', True), ('plain', False), ('bnact-relu', True), ('bnact-none', True))
POOLED_MODES = tuple(m for m in FWD_MODES if m[1])      # (the pooled sums are checked against the statistics' own values)
SE_MODES = (('se_pre', True), ('se_post', True))
BWD_MODES = ('plain_res', 'bnact', 'bnact_ps')            # bnact: hswish, the three modes of test_dwconv_bwd
BWD_ACT_MODES = BWD_MODES + ('bnact-relu6', 'bnact-relu')   # and the other compile-time activations of the backward kernels


def _fwd(family, k, strides, dtypes, shapes, pooled, forced, modes=FWD_MODES, passes=1):
    """One row per (dtype, stride, shape[, pass]); the mode walks round `modes`, starting one further for every (dtype, stride), so
    a cell with few shapes still meets every mode over its strides.  pooled: 0 | 1 | 'alt' (every other row)."""
    rows, start = [], 0
    for dt, s in itertools.product(dtypes, strides):
        for i, (B, C, H, W) in enumerate(shapes * passes):
            mode, stats = modes[(start + i) % len(modes)]
            p = (i + start) % 2 if pooled == 'alt' else pooled
            rows.append(Case('fwd', family, dt, B, C, H, W, k, s, int(bool(p and stats)), int(mode.startswith('se')), forced,
                             mode, stats))
        start += 1
    return rows


_walk = itertools.count()


def _bwd(family, k, strides, shapes, forced, every_mode=False, passes=1):
    """One row per (dtype, stride, shape) with the mode walking on round BWD_ACT_MODES from group to group, or one per
    (dtype, stride, shape, mode of BWD_MODES) with every_mode."""
    rows = []
    for dt, s in itertools.product(TRAIN, strides):
        for B, C, H, W in shapes * passes:
            for mode in (BWD_MODES if every_mode else (BWD_ACT_MODES[next(_walk) % len(BWD_ACT_MODES)],)):
                rows.append(Case('bwd', family, dt, B, C, H, W, k, s, 0, 0, forced, mode, mode != 'plain_res'))
    return rows


CASES = (
    # ---- forward, 3x3 ------------------------------------------------------------------------------------------------------
    _fwd('ROW3', 3, (1, 2), ALL, S3, 0, False)
    + _fwd('TILE', 3, (1,), TRAIN, (P2, SLAB8, SLAB2), 1, False, POOLED_MODES)             # pooled, stride 1, up to 14x14: where the tiles are wanted
    + _fwd('TILE', 3, (1,), TRAIN, (ODD, CHUNK), 1, True, POOLED_MODES)
    + _fwd('TILE', 3, (2,), TRAIN, (ODD, CHUNK, P2), 1, True, POOLED_MODES)
    + _fwd('TILE', 3, (1, 2), TRAIN, S3_TILE, 0, True)
    + _fwd('ROWK', 3, (1,), TRAIN, (P1, ODD, CHUNK), 1, False, POOLED_MODES)
    + _fwd('ROWK', 3, (1,), ('f16',), S3, 1, False, POOLED_MODES)
    + _fwd('ROWK', 3, (2,), ALL, S3, 1, False, POOLED_MODES)
    + _fwd('ROWK', 3, (1, 2), ALL, S3, 0, True)
    + _fwd('LDS', 3, (1, 2), TRAIN, S3, 'alt', True)
    + _fwd('LDS', 3, (1, 2), TRAIN, S3, 'alt', False, SE_MODES)
    # ---- forward, 5x5 ------------------------------------------------------------------------------------------------------
    + _fwd('PLANE7', 5, (1,), TRAIN, (P7, P7B, P7C, P7L), 'alt', False, passes=2)
    + _fwd('TILE', 5, (1,), TRAIN, (T8, T913, MID, TALL2, TLOOP), 'alt', False)
    + _fwd('TILE', 5, (2,), TRAIN, (T8, T913, MID), 'alt', False)
    + _fwd('TILE', 5, (1,), TRAIN, (LONG, TALL, WIDE), 'alt', True)
    + _fwd('TILE', 5, (2,), TRAIN, (LONG, TALL2, WIDE, TLOOP), 'alt', True)
    + _fwd('ROWK', 5, (1,), ALL, (Q2, Q3, TALL, WIDE, CHUNK, LONG, W6, KSLAB, LOOP, KFLAT, KSLABS), 'alt', False)
    + _fwd('ROWK', 5, (2,), ALL, (Q2, Q3, TALL2, P7, TALL, CHUNK, W6, KSLAB, LOOP, KFLAT, KSLABS), 'alt', False)
    + _fwd('ROWK', 5, (1,), ('f16',), (MID, P7, T913), 'alt', False)
    + _fwd('ROWK', 5, (2,), ('f16',), (MID, T8, T913), 'alt', False)
    + _fwd('ROWK', 5, (1,), TRAIN, (MID, T913, T8, P7), 'alt', True)
    + _fwd('ROWK', 5, (2,), TRAIN, (MID, T913, T8), 'alt', True)
    + _fwd('LDS', 5, (1, 2), TRAIN, (Q2, Q3, T8, T913, P7, MID, TALL2, CHUNK, LDSH), 'alt', True)
    + _fwd('LDS', 5, (1, 2), TRAIN, (Q2, Q3, T913, MID, LDSH), 'alt', False, SE_MODES)
    # ---- backward ----------------------------------------------------------------------------------------------------------
    + _bwd('ROW3', 3, (1, 2), S3, False)
    + _bwd('TILE', 3, (1, 2), S3_TILE, True)
    + _bwd('LDS', 3, (1, 2), S3, True, every_mode=True)                      # no reference check at all before: every mode
    + _bwd('PLANE7', 5, (1,), (P7, P7B, P7C, P7L), False, passes=2)
    + _bwd('TILE', 5, (1,), (T8, T913, MID, TALL2, TLOOP), False)
    + _bwd('TILE', 5, (2,), (T8, T913, MID), False)
    + _bwd('TILE', 5, (1,), (LONG, TALL, WIDE), True)
    + _bwd('TILE', 5, (2,), (LONG, TALL2, WIDE, TLOOP), True)
    + _bwd('ROWK', 5, (1,), (Q2, Q3, TALL, WIDE, CHUNK, LONG, W6, KSLAB, LOOP, KFLAT, KSLABS), False)
    + _bwd('ROWK', 5, (2,), (Q2, Q3, TALL2, P7, TALL, CHUNK, W6, KSLAB, LOOP, KFLAT, KSLABS), False)
    + _bwd('ROWK', 5, (1,), (MID, T913, T8, P7), True)
    + _bwd('ROWK', 5, (2,), (MID, T913, T8), True)
    + _bwd('LDS', 5, (1, 2), (Q2, Q3, T8, T913, P7, MID, TALL2, CHUNK, LDSH), True, every_mode=True)
)


def case_id(c):
    return (f'{c.direction}-{c.family}{"!" if c.forced else ""}-{c.dtype}-{c.B}x{c.C}x{c.H}x{c.W}-k{c.k}s{c.stride}-{c.mode}'
            f'{"-pool" if c.pooled else ""}{"" if c.stats or c.direction == "bwd" else "-nostats"}')
