"""CPU checks of the depthwise dispatch: t3d_dwconv_route is a pure function of the call's shape (no device call), so which
kernel family a shape takes can be asked -- and pinned down -- without a GPU."""
import itertools

from torchdet3d import _native as N

TILE, ROW3, PLANE7, ROWK, LDS = N.DW_TILE, N.DW_ROW3, N.DW_PLANE7, N.DW_ROWK, N.DW_LDS
ARG, UNSUPPORTED = N.ERR_ARG, N.ERR_UNSUPPORTED
F32, BF16, F16 = N.F32, N.BF16, N.F16


def route(backward, k, s, H, W, C, dtype=BF16, B=2, gated=0, pooled=0):
    return N.lib().t3d_dwconv_route(backward, dtype, gated, pooled, B, H, W, C, k, s)


# (k, stride, H, W, C), keyword overrides -> route
FWD_ROWS = [
    ((3, 1, 14, 14, 480), dict(pooled=1), TILE),
    ((3, 1, 15, 14, 480), dict(pooled=1), ROWK),
    ((3, 2, 14, 14, 480), dict(pooled=1), ROWK),
    ((3, 1, 14, 14, 480), {}, ROW3),
    ((3, 1, 14, 14, 480), dict(pooled=1, dtype=F16), ROWK),
    ((3, 1, 24, 24, 32), dict(gated=1), LDS),
    ((5, 1, 7, 7, 960), {}, PLANE7),
    ((5, 1, 7, 7, 960), dict(dtype=F16), ROWK),
    ((5, 1, 8, 8, 40), {}, TILE),
    ((5, 1, 64, 64, 40), {}, TILE),
    ((5, 1, 65, 64, 40), {}, ROWK),
    ((5, 2, 28, 28, 120), {}, TILE),
    ((5, 2, 56, 56, 72), {}, ROWK),
    ((5, 1, 3, 3, 960), {}, ROWK),
    ((5, 1, 12, 12, 120), dict(gated=1), LDS),
    ((3, 1, 14, 14, 12), {}, ARG),
]
BWD_ROWS = [
    ((3, 1, 56, 56, 144), {}, ROW3),
    ((3, 1, 112, 112, 672), dict(B=128), LDS),
    ((3, 2, 112, 112, 672), dict(B=128), LDS),
    ((3, 1, 112, 112, 672), dict(B=64, dtype=F32), LDS),
    ((3, 1, 112, 112, 672), dict(B=63, dtype=F32), ROW3),
    ((5, 1, 7, 7, 960), {}, PLANE7),
    ((5, 1, 28, 28, 120), {}, TILE),
    ((5, 2, 14, 14, 672), {}, TILE),
    ((5, 2, 56, 56, 72), {}, ROWK),
    ((5, 1, 3, 3, 960), {}, ROWK),
    ((3, 1, 56, 56, 144), dict(gated=1), UNSUPPORTED),
    ((5, 1, 28, 28, 120), dict(gated=1), UNSUPPORTED),
    ((3, 1, 56, 56, 144), dict(dtype=F16), ARG),
    ((5, 1, 28, 28, 120), dict(dtype=F16), ARG),
    ((3, 1, 14, 14, 12), {}, ARG),
]


def _check_rows():
    for backward, rows in ((0, FWD_ROWS), (1, BWD_ROWS)):
        for shape, kw, want in rows:
            assert route(backward, *shape, **kw) == want, (backward, shape, kw)


def test_named_shapes_take_the_kernels_the_cascade_gave_them():
    _check_rows()


def _oracle(backward, dtype, g, p, B, H, W, C, k, s):
    """The routing rules, written out once and frozen: what the try-the-next-launcher cascade did for every call."""
    if B <= 0 or H <= 0 or W <= 0 or C <= 0 or C % 8:
        return ARG
    train = dtype in (F32, BF16)
    s12 = s in (1, 2)
    tile5 = k == 5 and s12 and all(8 <= v <= (28 if s == 2 else 64) for v in (H, W))
    if not backward:
        if k == 3 and p and not g and s == 1 and 2 <= H <= 14 and 2 <= W <= 14 and train:
            return TILE
        if k == 3 and not p and not g and s12:
            return ROW3
        if k == 5 and s == 1 and H == 7 and W == 7 and not g and train:
            return PLANE7
        if tile5 and not g and train:
            return TILE
        if k in (3, 5) and s12 and not g:
            return ROWK
        if train and k in (3, 5) and s12:
            return LDS
        return UNSUPPORTED if train else ARG
    if g:
        return UNSUPPORTED
    if not train:
        return ARG
    if k == 3 and s12:
        return ROW3 if B * H * W * C * (4 if dtype == F32 else 2) < 2 ** 31 else LDS
    if k == 5 and s == 1 and H == 7 and W == 7:
        return PLANE7
    if tile5:
        return TILE
    if k == 5 and s12:
        return ROWK
    return LDS if k in (3, 5) and s12 else UNSUPPORTED


def test_every_shape_of_the_grid_routes_as_the_frozen_rules_say():
    fn = N.lib().t3d_dwconv_route
    sides = (1, 2, 3, 7, 8, 14, 15, 28, 29, 56, 64, 65)
    n = 0
    for backward, k, s, H, W, C, dtype, p, g, B in itertools.product((0, 1), (3, 5), (1, 2), sides, sides, (8, 24, 72, 960),
                                                                     (F32, BF16, F16), (0, 1), (0, 1), (1, 256)):
        got = fn(backward, dtype, g, p, B, H, W, C, k, s)
        assert got == _oracle(backward, dtype, g, p, B, H, W, C, k, s), (backward, dtype, g, p, B, H, W, C, k, s)
        if dtype != F16 and not (backward and g):
            assert got >= 0
        n += 1
    assert n == 2 * 2 * 2 * 12 * 12 * 4 * 3 * 2 * 2 * 2


OPT_IN_3X3 = [(2, 32, 24, 24, 3, 1), (2, 96, 24, 24, 3, 2), (5, 264, 9, 7, 3, 1), (3, 40, 13, 17, 3, 2), (2, 960, 7, 7, 3, 1)]   # B, C, H, W, k, s


def test_a_forced_route_is_taken_wherever_its_kernels_can_and_refused_elsewhere():
    force = N.lib().t3d_dwconv_force_route
    try:
        assert force(TILE) == 0
        for (B, C, H, W, k, s), dtype, backward in itertools.product(OPT_IN_3X3, (F32, BF16), (0, 1)):
            assert route(backward, k, s, H, W, C, dtype=dtype, B=B) == TILE
        for backward in (0, 1):
            assert route(backward, 3, 1, 1, 1, 32) == UNSUPPORTED
            assert route(backward, 5, 1, 1, 1, 32) == UNSUPPORTED
        assert force(PLANE7) == 0
        for backward in (0, 1):
            assert route(backward, 3, 1, 7, 7, 960) == UNSUPPORTED
            assert route(backward, 5, 1, 7, 7, 960) == PLANE7
        assert force(LDS + 1) == ARG and force(-2) == ARG       # (and the forced route stays as it was)
        assert route(0, 5, 1, 7, 7, 960) == PLANE7
    finally:
        assert force(N.DW_AUTO) == 0
    _check_rows()


# ---- the parity case table (tests/dw_cases.py): every row reaches the family it names, no cell of a family is left without rows

FAMILY = dict(TILE=TILE, ROW3=ROW3, PLANE7=PLANE7, ROWK=ROWK, LDS=LDS)
DTYPE = dict(f32=F32, bf16=BF16, f16=F16)


def _row_route(c):
    return route(c.direction == 'bwd', c.k, c.stride, c.H, c.W, c.C, dtype=DTYPE[c.dtype], B=c.B, gated=c.gated, pooled=c.pooled)


def _cells():
    """Every (direction, family, k, stride, dtype) for which the family's `can` accepts some call of the sweep's grid: the
    forced route asks `can` alone."""
    force = N.lib().t3d_dwconv_force_route
    sides = (1, 2, 3, 7, 8, 14, 15, 28, 29, 56, 64, 65)
    cells = set()
    try:
        for name, fam in FAMILY.items():
            assert force(fam) == 0
            for backward, k, s, dtype in itertools.product((0, 1), (3, 5), (1, 2), DTYPE):
                if any(route(backward, k, s, H, W, C, dtype=DTYPE[dtype], B=B, gated=g, pooled=p) == fam
                       for H, W, C, p, g, B in itertools.product(sides, sides, (8, 24, 72, 960), (0, 1), (0, 1), (1, 256))):
                    cells.add((('fwd', 'bwd')[backward], name, k, s, dtype))
    finally:
        assert force(N.DW_AUTO) == 0
    return cells


def test_every_parity_case_reaches_the_family_it_names():
    from dw_cases import CASES
    force = N.lib().t3d_dwconv_force_route
    assert len(set(CASES)) == len(CASES)
    for c in CASES:
        assert c.direction in ('fwd', 'bwd') and c.family in FAMILY and c.dtype in DTYPE
        # what the GPU test passes follows from the row: gap_sum from `pooled`, the gate from the mode, no pooled sums without statistics
        assert c.gated == int(c.mode.startswith('se')) and (c.stats or not c.pooled) and (c.direction == 'fwd' or not c.pooled)
        auto = _row_route(c)
        if not c.forced:
            assert auto == FAMILY[c.family], c
        else:
            assert auto >= 0 and auto != FAMILY[c.family], c       # (a forced row the dispatcher sends there anyway is mislabelled)
            try:
                assert force(FAMILY[c.family]) == 0
                assert _row_route(c) == FAMILY[c.family], c
            finally:
                assert force(N.DW_AUTO) == 0


def test_every_cell_of_every_family_has_parity_cases():
    from dw_cases import BWD_ACT_MODES, BWD_MODES, CASES
    cells = _cells()
    assert (sum(c[0] == 'fwd' for c in cells), sum(c[0] == 'bwd' for c in cells)) == (36, 26)
    rows = {}
    for c in CASES:
        rows.setdefault((c.direction, c.family, c.k, c.stride, c.dtype), []).append(c)
    assert set(rows) <= cells                                        # (a row outside every `can` would have failed the test above)
    for cell in sorted(cells):
        assert len(rows.get(cell, ())) >= 2, cell
    fwd_fd = {(c[1], c[4]) for c in cells if c[0] == 'fwd'}
    for fam, dt in sorted(fwd_fd):
        mine = [c for c in CASES if c.direction == 'fwd' and (c.family, c.dtype) == (fam, dt)]
        modes = {c.mode for c in mine}
        assert {'plain', 'bnact-none', 'bnact-relu', 'bnact-relu6', 'bnact-hswish'} <= modes, (fam, dt)
        assert ({'se_pre', 'se_post'} <= modes) == (fam == 'LDS'), (fam, dt)
        assert any(not c.stats and not c.pooled for c in mine), (fam, dt)
        # pooled sums: every family but the 3x3 row walk takes them
        assert {c.pooled for c in mine} == ({0} if fam == 'ROW3' else {0, 1}), (fam, dt)
    # the packed clamp form of ReLU6: bf16 at stride 2 in the 3x3 row walk (stride 1: the column-pair kernel's own)
    for s in (1, 2):
        assert any(c.mode == 'bnact-relu6' for c in rows[('fwd', 'ROW3', 3, s, 'bf16')])
    for fam in {c[1] for c in cells if c[0] == 'bwd'}:
        for dt in ('f32', 'bf16'):
            modes = {c.mode for c in CASES if c.direction == 'bwd' and (c.family, c.dtype) == (fam, dt)}
            # (the LDS tiles take the activation as a run-time argument of the functions every family shares)
            assert modes == set(BWD_MODES if fam == 'LDS' else BWD_ACT_MODES), (fam, dt)
    # the 3x3 row walk instantiates its backward kernels per activation (bf16 ReLU6: the packed clamp form, at either stride)
    for cell in cells:
        if cell[:2] == ('bwd', 'ROW3'):
            assert {'bnact', 'bnact-relu6', 'bnact-relu', 'plain_res'} <= {c.mode for c in rows[cell]}, cell
    # the LDS-tiled backward: every mode in every cell
    for cell in cells:
        if cell[:2] == ('bwd', 'LDS'):
            assert {c.mode for c in rows[cell]} == set(BWD_MODES), cell
