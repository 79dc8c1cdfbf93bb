"""CPU checks of the row-walk launch planner: t3d_dwconv_plan is a pure function of the call's shape (no device call), so the
geometry every T3D_DW_ROW3 / T3D_DW_ROWK launch takes -- row chunks, flat or slab lane mapping, persistent grid, weight-gradient
slots, LDS bytes, template variant -- can be pinned down without a GPU.  The oracle below is the arithmetic of the six launchers
as they stood before they shared one planner, written out once and frozen."""
import ctypes
import itertools

from torchdet3d import _native as N

from test_dw_route import _oracle as route_oracle

ROW3, ROWK = N.DW_ROW3, N.DW_ROWK
F32, BF16, F16 = N.F32, N.BF16, N.F16
NTH = 256


def cdiv(a, b):
    return (a + b - 1) // b


def _walk(B, C, CH, rows, chunk_cols, grid_cols, want, min_rows, target, waste_pct, lds_per_channel, lds_whole=False,
          lds_must_fit=False, variant=None):
    """One launcher: (rows_per_chunk, nchunks, slab, nitems, grid.x, grid.y, slots_needed, LDS bytes, variant)"""
    CG = C // CH
    nchunks = cdiv(want, B * chunk_cols * CG)
    nchunks = max(1, min(nchunks, max(1, rows // min_rows)))
    rows_per_chunk = cdiv(rows, nchunks)
    nchunks = cdiv(rows, rows_per_chunk)
    slab_lanes = cdiv(CG, 64) * 64
    flat = CG < 64 or (waste_pct is not None and (slab_lanes - CG) * 100 > waste_pct * slab_lanes)
    if flat and CG >= 64 and lds_must_fit and lds_per_channel * C > 64 * 1024:
        flat = False
    if flat:
        nitems = B * nchunks
        jb = cdiv(grid_cols * CG, NTH)
        gx, gy = jb, max(1, min(target // jb, nitems))
        slots = gx * gy
    else:
        nitems = grid_cols * B * nchunks
        ns = cdiv(CG, 64)
        gx, gy = max(1, min(target // ns, cdiv(nitems, NTH // 64))), ns
        slots = gx
    lds = lds_per_channel * (C if (flat or lds_whole) else 64 * CH)
    return (rows_per_chunk, nchunks, int(not flat), nitems, gx, gy, slots, lds, CH if variant is None else variant)


def plan_oracle(route, backward, itemsize, B, H, W, C, k, s):
    """The six rows of the launchers' table."""
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1          # (pad (k - 1) / 2, either stencil)
    if route == ROW3 and not backward:                    # dwconv3_stream.hip: launch
        use2 = s == 1 and B * H * W * C * itemsize < 2 ** 31
        return _walk(B, C, 4, Ho, Wo, (Wo + 1) // 2 if use2 else Wo, 256 * 64 * 40, 8, 512 if (s == 1 and H > 28) else 768,
                     None, 16, lds_whole=True)
    if route == ROW3 and s == 1:                          # dwconv3_bwd_stream.hip: launch_s1c<CH>
        CH = 2 if C % 2 == 0 else 4
        return _walk(B, C, CH, H, (W + 1) // 2, (W + 1) // 2, 256 * 64 * 24, 8, 512 if CH == 2 else 256, 12, 88)
    if route == ROW3:                                     # dwconv3_bwd_stream.hip: launch_s2
        return _walk(B, C, 4, Ho, Wo, Wo, 256 * 64 * 24, 4, 512, None, 88)
    if not backward:                                      # dwconvk_stream.hip: launch_nc<K, S, NC>
        NC = 4 if (s == 1 and Wo >= 4) else 1
        Wb = cdiv(Wo, NC)
        want = 256 * 64 * 6 if (k == 5 and s == 1 and NC > 1) else 256 * 64 * 40
        return _walk(B, C, 2, Ho, Wb, Wb, want, 8, 1024 if (k == 5 and s == 1) else 768, 8, 16, variant=NC)
    if s == 1:                                            # dwconv5_bwd_stream.hip: launch5_s1
        return _walk(B, C, 2, H, W, W, 256 * 64 * 24, 5, 512, 8, 216, lds_must_fit=True)
    return _walk(B, C, 2, Ho, Wo, Wo, 256 * 64 * 24, 4, 512, 8, 216, lds_must_fit=True)       # launch5_s2


def can(route, backward, dtype, pooled, B, H, W, C, k, s):
    """Where a forced row-walk route launches (ungated calls of valid shape)."""
    train = dtype in (F32, BF16)
    if route == ROW3:
        if backward:
            return k == 3 and train and B * H * W * C * (4 if dtype == F32 else 2) < 2 ** 31
        return k == 3 and not pooled
    return train and k == 5 if backward else k in (3, 5)


_OUT = (ctypes.c_int * 9)()


def plan(backward, k, s, H, W, C, dtype=BF16, B=2, pooled=0):
    r = N.lib().t3d_dwconv_plan(backward, dtype, 0, pooled, B, H, W, C, k, s, _OUT)
    return r, tuple(_OUT)


def forced(route):
    class _Forced:
        def __enter__(self):
            assert N.lib().t3d_dwconv_force_route(route) == 0

        def __exit__(self, *exc):
            assert N.lib().t3d_dwconv_force_route(N.DW_AUTO) == 0
    return _Forced()


def check(route, backward, k, s, H, W, C, dtype=BF16, B=2):
    """plan of one call under the forced route == the oracle; returns it as a dict"""
    with forced(route):
        r, got = plan(backward, k, s, H, W, C, dtype=dtype, B=B)
    assert r == route, (route, backward, k, s, H, W, C, dtype, B, r)
    assert got == plan_oracle(route, backward, 4 if dtype == F32 else 2, B, H, W, C, k, s), (route, backward, k, s, H, W, C, dtype, B)
    return dict(zip(('rows_per_chunk', 'nchunks', 'slab', 'nitems', 'gx', 'gy', 'slots', 'lds', 'variant'), got))


SIDES = (1, 2, 3, 4, 5, 7, 8, 14, 15, 28, 56, 112, 113)
PLANES = list(itertools.product(SIDES, SIDES)) + [(7, 14), (14, 7), (28, 3)]
CHANNELS = (8, 24, 64, 120, 128, 136, 248, 256, 264, 304, 312, 480, 576, 672, 960, 1152)
BATCHES = (1, 2, 8, 64, 256)


def _sweep(force):
    fn = N.lib().t3d_dwconv_plan
    zeros = (0,) * 9
    n = launched = 0
    for backward, k, s in itertools.product((0, 1), (3, 5), (1, 2)):
        for dtype in ((F32, BF16) if backward else (F32, BF16, F16)):
            itemsize = 4 if dtype == F32 else 2
            for pooled, B, (H, W), C in itertools.product((0, 1), BATCHES, PLANES, CHANNELS):
                r = fn(backward, dtype, 0, pooled, B, H, W, C, k, s, _OUT)
                got = tuple(_OUT)
                case = (force, backward, dtype, pooled, B, H, W, C, k, s)
                if force is None:
                    assert r == route_oracle(backward, dtype, 0, pooled and not backward, B, H, W, C, k, s), case
                else:       # no error where the entry point would launch, the family's own error where it would not
                    assert r == (force if can(force, backward, dtype, pooled and not backward, B, H, W, C, k, s) else N.ERR_UNSUPPORTED), case
                if r in (ROW3, ROWK):
                    assert got == plan_oracle(r, backward, itemsize, B, H, W, C, k, s), case
                    launched += 1
                else:
                    assert got == zeros, case
                n += 1
    assert n == (4 * 3 + 4 * 2) * 2 * len(BATCHES) * len(PLANES) * len(CHANNELS)
    return launched


def test_every_automatic_row_walk_launch_of_the_grid_has_the_frozen_geometry():
    assert _sweep(None) > 100000


def test_every_forced_row3_launch_of_the_grid_has_the_frozen_geometry():
    with forced(ROW3):
        assert _sweep(ROW3) > 100000


def test_every_forced_rowk_launch_of_the_grid_has_the_frozen_geometry():
    with forced(ROWK):
        assert _sweep(ROWK) > 100000


def test_other_routes_and_errors_fill_zeros():
    assert plan(0, 5, 1, 7, 7, 960) == (N.DW_PLANE7, (0,) * 9)
    assert plan(1, 5, 1, 28, 28, 120) == (N.DW_TILE, (0,) * 9)
    assert plan(0, 3, 1, 14, 14, 12) == (N.ERR_ARG, (0,) * 9)
    assert N.lib().t3d_dwconv_plan(0, BF16, 0, 0, 2, 14, 14, 16, 3, 1, None) == N.ERR_ARG


def test_576_channels_backward_take_slabs_by_either_rule():
    # 3x3 stride 1: 288 channel pairs in 5 slabs waste 10 % of the lanes, under the 12 % rule -> slabs of 128 channels
    p = check(ROW3, 1, 3, 1, 14, 14, 576, B=256)
    assert (p['slab'], p['gy'], p['lds'], p['variant']) == (1, 5, 22 * 128 * 4, 2)
    # 5x5: 10 % is over the 8 % rule -> flat, but 54 * 576 * 4 B of scratch pass 64 KiB -> slabs after all
    for s in (1, 2):
        p = check(ROWK, 1, 5, s, 14, 14, 576, B=256)
        assert (p['slab'], p['gy'], p['lds']) == (1, 5, 54 * 128 * 4)
    # the k x k forward has the 8 % rule and no LDS rule: flat
    p = check(ROWK, 0, 5, 1, 14, 14, 576, B=256)
    assert (p['slab'], p['lds']) == (0, 16 * 576)


def test_64_channel_groups_are_the_first_slab():
    # 2 channels per thread: C = 128; 4 channels per thread: C = 256
    for route, backward, k, s, C in ((ROW3, 1, 3, 1, 128), (ROWK, 0, 3, 1, 128), (ROWK, 0, 5, 2, 128), (ROWK, 1, 5, 1, 128),
                                     (ROWK, 1, 5, 2, 128), (ROW3, 0, 3, 1, 256), (ROW3, 0, 3, 2, 256), (ROW3, 1, 3, 2, 256)):
        at, below = check(route, backward, k, s, 28, 28, C, B=8), check(route, backward, k, s, 28, 28, C - 8, B=8)
        assert (at['slab'], at['gy'], below['slab']) == (1, 1, 0), (route, backward, k, s, C)
    # (4 channels per thread at C = 128 is still flat)
    assert check(ROW3, 0, 3, 1, 28, 28, 128, B=8)['slab'] == 0


def test_flat_5x5_backward_scratch_stops_at_64_kib():
    # all three waste > 8 % of their slabs' lanes; 54 * 4 * C bytes of flat scratch: 63936 at C = 296, 65664 at 304
    for s in (1, 2):
        assert check(ROWK, 1, 5, s, 14, 14, 296)['slab'] == 0 and check(ROWK, 1, 5, s, 14, 14, 296)['lds'] == 216 * 296
        for C in (304, 312):
            p = check(ROWK, 1, 5, s, 14, 14, C)
            assert (p['slab'], p['gy'], p['lds']) == (1, 3, 216 * 128), (s, C)
    # the 3x3 backward has the waste rule alone: flat at either
    for C in (304, 312):
        assert check(ROW3, 1, 3, 1, 14, 14, C)['slab'] == 0


def test_3x3_forward_walks_single_columns_from_2_gib_and_still_counts_chunks_in_columns():
    below, above = check(ROW3, 0, 3, 1, 112, 112, 328, B=256), check(ROW3, 0, 3, 1, 112, 112, 336, B=256)
    assert 256 * 112 * 112 * 328 * 2 < 2 ** 31 <= 256 * 112 * 112 * 336 * 2
    assert below['slab'] == above['slab'] == 1
    assert (below['rows_per_chunk'], below['nchunks']) == (above['rows_per_chunk'], above['nchunks'])
    assert below['nitems'] == 56 * 256 * below['nchunks'] and above['nitems'] == 112 * 256 * above['nchunks']
    # stride 2 never pairs columns
    assert check(ROW3, 0, 3, 2, 112, 112, 328, B=2)['nitems'] == 56 * 2 * check(ROW3, 0, 3, 2, 112, 112, 328, B=2)['nchunks']


def test_fewer_rows_than_the_shortest_chunk_make_one_chunk():
    for route, backward, k, s, H in ((ROW3, 0, 3, 1, 7), (ROW3, 0, 3, 2, 14), (ROW3, 1, 3, 1, 7), (ROW3, 1, 3, 2, 5),
                                     (ROWK, 0, 5, 1, 7), (ROWK, 0, 3, 2, 13), (ROWK, 1, 5, 1, 4), (ROWK, 1, 5, 2, 5)):
        p = check(route, backward, k, s, H, 5, 24, B=1)
        assert (p['nchunks'], p['rows_per_chunk']) == (1, (H - 1) // s + 1), (route, backward, k, s, H)


def test_rows_narrower_than_four_outputs_take_one_column_per_thread():
    for k in (3, 5):
        assert check(ROWK, 0, k, 1, 8, 3, 64)['variant'] == 1
        assert check(ROWK, 0, k, 1, 8, 4, 64)['variant'] == 4
        assert check(ROWK, 0, k, 2, 8, 112, 64)['variant'] == 1
