"""CPU checks of the pointwise (1x1) dispatch: t3d_pwconv_route is a pure function of the call's dtype, options and sizes (no
device call), so which kernel family a call takes can be asked -- and pinned down -- without a GPU."""
import ctypes
import itertools

from torchdet3d import _native as N

DEEP, STREAM, REG32, LDS, TR, PAIR = N.PW_DEEP, N.PW_STREAM, N.PW_REG32, N.PW_LDS, N.PW_TR, N.PW_PAIR
FWD, FWD_STATS, MAT, DGRAD, WGRAD = N.PW_OP_FWD, N.PW_OP_FWD_STATS, N.PW_OP_MAT, N.PW_OP_DGRAD, N.PW_OP_WGRAD
ARG, UNSUPPORTED = N.ERR_ARG, N.ERR_UNSUPPORTED
F32, BF16, F16 = N.F32, N.BF16, N.F16
FRAG = N.W_FRAG
WS_BYTES = 64 << 20


def route(op, K, N_, M, HW, dtype=BF16, gated=0, per_sample=0, ps_stats=0, e_se=0, bias=0, stats=0, alpha_gamma=1, act=0,
          residual=0):
    return N.lib().t3d_pwconv_route(op, dtype, gated, per_sample, ps_stats, e_se, bias, stats, alpha_gamma, act, residual, M, HW,
                                    K, N_)


class workspace:
    """t3d_set_workspace with an address that is never read: the fp32 weight gradient's route asks only for its size."""

    def __init__(self, nbytes):
        self.nbytes = nbytes

    def __enter__(self):
        assert N.lib().t3d_set_workspace(ctypes.c_void_p(4096 if self.nbytes else None), self.nbytes) == 0

    def __exit__(self, *exc):
        assert N.lib().t3d_set_workspace(None, 0) == 0


B = 256
# (op, K, N, M, HW), keyword overrides -> route          (MobileNetV2 / V3 layers at B = 256)
ROWS = [
    ((FWD, 32, 16, B * 112 * 112, 112 * 112), dict(stats=1), STREAM),
    ((FWD_STATS, 16, 96, B * 112 * 112, 112 * 112), dict(stats=1), STREAM),
    ((FWD, 96, 576, B * 196, 196), dict(stats=1), STREAM),
    ((MAT, 576, 96, B * 196, 196), dict(stats=1, residual=1), STREAM),
    ((MAT, 576, 96, B * 196, 196), dict(stats=1, dtype=BF16 | FRAG), STREAM),
    ((DGRAD, 96, 576, B * 196, 196), dict(stats=1), STREAM),                      # contraction over 576: one 96-channel chunk
    ((DGRAD, 576, 96, B * 196, 196), dict(stats=1, dtype=BF16 | FRAG), STREAM),
    ((FWD, 960, 160, B * 49, 49), dict(stats=1, dtype=BF16 | FRAG), DEEP),
    ((FWD, 960, 160, B * 49, 49), dict(stats=1), STREAM),                         # row-major weights: not the deep kernel
    ((DGRAD, 160, 960, B * 49, 49), dict(stats=1, dtype=BF16 | FRAG), DEEP),
    ((FWD, 960, 160, B * 49, 49), dict(stats=1, gated=1, dtype=BF16 | FRAG), STREAM),   # a gated projection
    ((DGRAD, 672, 160, B * 49, 49), dict(ps_stats=1, e_se=1, dtype=BF16 | FRAG), STREAM),
    ((FWD, 2048, 512, B * 49, 49), dict(stats=1), LDS),
    ((FWD, 2048, 512, B * 49, 49), dict(stats=1, dtype=BF16 | FRAG), DEEP),
    ((FWD, 2048, 512, B * 49, 49), dict(stats=1, gated=1, dtype=BF16 | FRAG), UNSUPPORTED),
    ((WGRAD, 96, 576, B * 196, 196), {}, TR),
    ((WGRAD, 96, 576, B * 196, 196), dict(per_sample=1, gated=1), TR),
    ((FWD, 320, 1280, B * 49, 49), dict(stats=1, dtype=F32), REG32),
    ((FWD, 1280, 9, B, 1), dict(dtype=F32), ARG),
    ((FWD, 1280, 16, B, 1), dict(bias=1, dtype=F32), LDS),                        # the classifier: M = 256, the split contraction
    ((DGRAD, 1280, 16, B, 1), dict(dtype=F32), LDS),
    ((MAT, 576, 96, B * 196, 196), dict(stats=1, dtype=F32), REG32),
    ((MAT, 576, 96, 2 * 196, 196), dict(stats=1, dtype=F32), PAIR),
    ((MAT, 576, 96, B * 196, 196), dict(stats=1, dtype=F32, act=2), PAIR),
    ((MAT, 576, 96, B * 196, 196), dict(dtype=F16), PAIR),
    ((MAT, 576, 96, B * 196, 196), dict(dtype=F16 | FRAG), ARG),
    ((MAT, 2048, 512, B * 49, 49), dict(dtype=BF16 | FRAG), UNSUPPORTED),
    ((MAT, 2048, 512, B * 49, 49), {}, PAIR),
    ((MAT, 576, 96, B * 196, 196), dict(gated=1), ARG),
    ((WGRAD, 96, 576, B * 196, 196), dict(dtype=F32), LDS),                       # (no workspace)
    ((FWD, 96, 576, B * 196, 196), dict(dtype=F16, gated=1), STREAM),
    ((FWD, 96, 576, B * 196, 196), dict(dtype=F16, stats=1), UNSUPPORTED),
    ((DGRAD, 96, 576, B * 196, 196), dict(dtype=F16), UNSUPPORTED),
    ((WGRAD, 96, 576, B * 196, 196), dict(dtype=F16), ARG),
    ((WGRAD, 96, 576, B * 196, 196), dict(dtype=BF16 | FRAG), ARG),
    ((FWD, 96, 576, B * 196, 196), dict(dtype=F32 | FRAG), ARG),
    ((FWD_STATS, 96, 576, B * 196, 196), dict(dtype=F32, stats=1), UNSUPPORTED),
    ((FWD, 96, 12, B * 196, 196), {}, ARG),
]


def _check_rows():
    for shape, kw, want in ROWS:
        assert route(*shape, **kw) == want, (shape, kw)


def test_named_shapes_take_the_kernels_the_cascade_gave_them():
    _check_rows()
    with workspace(WS_BYTES):
        assert route(WGRAD, 96, 576, B * 196, 196, dtype=F32) == REG32
        assert route(WGRAD, 96, 576, B * 196, 196, dtype=F32, gated=1) == LDS
    with workspace(15 << 20):                                               # 56 splits of 18 tiles of 64 x 64: 15.75 MB of partials
        assert route(WGRAD, 96, 576, B * 196, 196, dtype=F32) == LDS


def _cdiv(a, b):
    return -(-a // b)


def _deep_can(Kin, Nout):
    """pwconv_deep.hip: the shapes where the streaming kernel needs more than one output chunk, inside 150 KB of LDS"""
    if Kin < 512:
        return False
    KS = _cdiv(Kin, 32)
    cap = min(120 // KS, 10) & ~1
    if cap >= 2 and Nout <= cap * 16:
        return False
    pairs = _cdiv(Nout, 32)
    ntiles = 2 * _cdiv(pairs, _cdiv(pairs, 8))
    return 2 * 4 * 4 * 1024 + 3 * KS * 32 * 4 + ntiles * 16 * 24 <= 150 * 1024


def _reg32_grid(dgrad, stats, residual, gated, M, Nout):
    """pwconv_f32_reg.hip: workgroups of the launch"""
    tiles, G = _cdiv(Nout, 16), _cdiv(M, 16)
    NT = 2
    if tiles > 2:
        pad = 1 << 30
        for n in (5, 4, 6, 3):
            if _cdiv(tiles, n) * n < pad:
                pad, NT = _cdiv(tiles, n) * n, n
    nchunks = _cdiv(tiles, NT)
    R = 4 if _cdiv(_cdiv(G, 4), 4) * nchunks >= 128 else 2
    if R == 4 and NT > 4 and (dgrad or (stats and (NT == 6 or residual)) or gated):
        R = 2
    npw = _cdiv(_cdiv(_cdiv(G, R), 4), 8) * 8
    if stats or dgrad:
        npw = min(npw, max(8, 512 // nchunks // 8 * 8))
    return npw * nchunks


def _wg32_bytes(M, K, N_):
    """pwconv_f32_wgrad.hip: bytes of partial tiles"""
    tn, tk = _cdiv(N_, 64), _cdiv(K, 64)
    sel = 0
    for k in (3, 2, 1):
        sg = 256 * k // (tn * tk)
        if not sel and sg >= 1 and (M // (4 * sg) >= 512 or k == 1):
            sel = sg
    S = 4 * (sel or 1)
    S = max(min(S, _cdiv(M, 512)), 4)
    S = (S + 3) & ~3
    rows = _cdiv(_cdiv(M, S), 24) * 24
    return _cdiv(_cdiv(M, rows), 4) * 4 * tn * tk * 64 * 64 * 4


def _oracle(op, dtype, gated, per_sample, ps_stats, e_se, bias, stats, alpha_gamma, act, residual, M, HW, K, N_, ws=0, forced=-1):
    """The routing rules, written out once and frozen: what the try-the-next-launcher cascades did for every call."""
    wfrag, dtype = bool(dtype & FRAG), dtype & ~FRAG
    bwd, dg = op in (DGRAD, WGRAD), op == DGRAD
    # flags the operation's entry point has no argument for
    gated = gated and not dg
    per_sample, alpha_gamma = per_sample and bwd, alpha_gamma and bwd
    ps_stats, e_se = ps_stats and dg, e_se and dg
    bias, stats, residual = bias and op in (FWD, FWD_STATS), stats and op != WGRAD, residual and op == MAT
    act = 0 if bwd else act
    Kin, Nout = (N_, K) if bwd else (K, N_)
    sizes = M > 0 and HW > 0 and Kin > 0 and Nout > 0 and Kin % 8 == 0 and Nout % 8 == 0
    gen = per_sample or ps_stats or e_se or (not dg and gated)
    stream16 = sizes and dtype == BF16 and op != WGRAD and Kin <= 1920 and not (ps_stats and (stats or M % HW)) \
        and not (op == MAT and gated)
    if op == FWD_STATS:
        return STREAM if stream16 and forced in (-1, STREAM) else UNSUPPORTED
    if not sizes or dtype not in (F32, BF16, F16):
        return ARG
    if (wfrag and dtype == F32) or (op == MAT and gated) or (op == WGRAD and (wfrag or dtype == F16)):
        return ARG
    can = {
        DEEP: dtype == BF16 and wfrag and op in (FWD, DGRAD) and not gen and not bias and (not dg or alpha_gamma)
        and _deep_can(Kin, Nout),
        STREAM: stream16 or (dtype == F16 and op == FWD and not stats and Kin <= 1920),
        LDS: (dtype in (F32, BF16) and not wfrag and op in (FWD, DGRAD)) or (dtype == F32 and op == WGRAD),
        TR: dtype == BF16 and op == WGRAD,
    }
    if op == WGRAD:
        can[REG32] = dtype == F32 and not per_sample and not gated and M >= 1024 and alpha_gamma and ws >= _wg32_bytes(M, K, N_)
    else:
        can[REG32] = dtype == F32 and M >= 1024 and (op == FWD or (op == MAT and act == 0) or
                                                     (dg and alpha_gamma and not (per_sample or ps_stats or e_se))) \
            and _reg32_grid(dg, stats, residual, gated, M, Nout) < 2 ** 31
    pair = op == MAT and not wfrag
    if forced != -1:
        return forced if can[forced] else (PAIR if pair else UNSUPPORTED)
    for r in (DEEP, STREAM, REG32, TR, LDS):
        if can[r]:
            return r
    if pair:
        return PAIR
    return ARG if op == MAT and dtype != BF16 else UNSUPPORTED


OPS = (FWD, FWD_STATS, MAT, DGRAD, WGRAD)
MS, HWS, CH = (8, 1023, 1024, 50176), (1, 49, 64), (8, 32, 64, 160, 512, 960, 1920, 1928)


def _sweep(forced=-1, ms=MS, hws=HWS, ch=CH):
    fn = N.lib().t3d_pwconv_route
    n = 0
    for ws in (0, WS_BYTES):
        with workspace(ws):
            for op in OPS if ws == 0 else (WGRAD,):
                for dtype, wfrag, M, HW, K, N_, g, p, pss, st, b in itertools.product(
                        (F32, BF16, F16), (0, FRAG), ms, hws, ch, ch, (0, 1), (0, 1), (0, 1), (0, 1), (0, 1)):
                    got = fn(op, dtype | wfrag, g, p, pss, 0, b, st, 1, 0, 0, M, HW, K, N_)
                    assert got == _oracle(op, dtype | wfrag, g, p, pss, 0, b, st, 1, 0, 0, M, HW, K, N_, ws, forced), \
                        (op, dtype, wfrag, g, p, pss, b, st, M, HW, K, N_, ws, forced)
                    n += 1
    return n


def test_every_call_of_the_grid_routes_as_the_frozen_rules_say():
    assert _sweep() == 6 * 3 * 2 * 4 * 3 * 8 * 8 * 32


def test_the_options_outside_the_grid_and_bad_sizes_route_as_the_frozen_rules_say():
    fn = N.lib().t3d_pwconv_route
    shapes = [(50176, 196, 96, 576), (50176, 196, 576, 96), (12544, 49, 960, 160), (12544, 49, 160, 960), (256, 1, 1280, 16),
              (50176, 196, 96, 12), (50176, 196, 12, 96), (0, 196, 96, 576), (50176, 0, 96, 576), (50176, 196, 0, 576),
              (2 ** 30, 1, 8, 2 ** 30)]
    for (M, HW, K, N_), op, dtype, e_se, ag, act, res, st, g in itertools.product(
            shapes, OPS, (F32, BF16, BF16 | FRAG, F16, 7), (0, 1), (0, 1), (0, 2, 3), (0, 1), (0, 1), (0, 1)):
        args = (op, dtype, g, 0, 0, e_se, 0, st, ag, act, res, M, HW, K, N_)
        assert fn(*args) == _oracle(*args), args
    assert fn(5, BF16, 0, 0, 0, 0, 0, 0, 1, 0, 0, 64, 16, 32, 32) == ARG and fn(-1, BF16, 0, 0, 0, 0, 0, 0, 1, 0, 0, 64, 16, 32, 32) == ARG


def test_a_forced_route_is_taken_wherever_its_kernels_can_and_refused_elsewhere():
    force = N.lib().t3d_pwconv_force_route
    big = (B * 196, 196)
    try:
        assert force(LDS) == 0
        # every fp32 call: the LDS-tiled kernels, and the materialising forward as its two launches
        for M in (256, 50176):
            assert route(FWD, 96, 576, M, 196, dtype=F32, stats=1) == LDS
            assert route(DGRAD, 96, 576, M, 196, dtype=F32, stats=1) == LDS
            assert route(MAT, 576, 96, M, 196, dtype=F32, stats=1) == PAIR
            with workspace(WS_BYTES):
                assert route(WGRAD, 96, 576, M, 196, dtype=F32) == LDS
        assert route(FWD, 96, 576, *big) == LDS and route(MAT, 576, 96, *big) == PAIR
        assert route(FWD, 96, 576, *big, dtype=BF16 | FRAG) == UNSUPPORTED
        assert route(MAT, 576, 96, *big, dtype=BF16 | FRAG) == UNSUPPORTED
        assert route(WGRAD, 96, 576, *big) == UNSUPPORTED and route(FWD, 96, 576, *big, dtype=F16) == UNSUPPORTED
        assert route(FWD_STATS, 16, 96, *big, stats=1) == UNSUPPORTED
        assert route(FWD, 96, 12, *big) == ARG                                   # (validation comes first)
        assert force(DEEP) == 0
        assert route(FWD, 64, 32, 64, 16) == UNSUPPORTED
        assert route(FWD, 64, 32, 64, 16, dtype=BF16 | FRAG) == UNSUPPORTED
        assert route(FWD, 960, 160, B * 49, 49, dtype=BF16 | FRAG) == DEEP
        assert route(FWD, 960, 160, B * 49, 49) == UNSUPPORTED
        assert force(STREAM) == 0
        assert route(FWD, 960, 160, B * 49, 49, dtype=BF16 | FRAG) == STREAM
        assert route(FWD, 96, 576, *big, dtype=F32) == UNSUPPORTED
        assert force(REG32) == 0
        assert route(FWD, 1280, 16, 256, 1, dtype=F32) == UNSUPPORTED and route(MAT, 576, 96, 392, 196, dtype=F32) == PAIR
        assert force(PAIR) == ARG and force(-2) == ARG       # (and the forced route stays as it was)
        assert route(FWD, 96, 576, *big, dtype=F32) == REG32
        for r in (DEEP, STREAM, REG32, LDS, TR):
            assert force(r) == 0
            assert _sweep(r, ms=(8, 1024), hws=(49,), ch=(8, 64, 960, 1928)) == 6 * 3 * 2 * 2 * 16 * 32
    finally:
        assert force(N.PW_AUTO) == 0
    _check_rows()
