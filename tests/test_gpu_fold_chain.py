"""BatchNorm finalize derived in the consumer's prologue (csrc/common.h: t3d_fold_block) and the statistics tail of the bf16
streaming pointwise kernel (csrc/pwconv_stream.hip), held to BYTES:

  * a launch that serves a t3d_fold_request publishes byte for byte what the standalone t3d_bn_finalize / t3d_bn_bwd_finalize
    launch writes (kind 1: also running mean, running variance and the batch counter) and produces byte for byte the outputs
    of finalize + the plain launch -- for every replica count the derive treats differently (1, 2, 3: surplus slots of the
    4-replica body; 8; 16) and channel counts that leave a wave partly (8, 24, 72, 200) or wholly (every wave of the block
    past the first) without channels, and once per kernel family that has a derive prologue;
  * the BatchNorm sums a streaming launch leaves are byte-equal to the values recorded in tests/golden/fold_chain_sums.npz.

The fixture was written by `T3D_LIB=<libt3d_hip.so of the commit before the tail changed> python tests/test_gpu_fold_chain.py
--write-golden` on an MI355X: the operands below are integer patterns (no random generator involved), so the same call on
any build adds the same numbers."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'fold_chain_sums.npz')
BF = torch.bfloat16
MOM, EPS = 0.1, 1e-5


def _raw(t):
    return t.detach().contiguous().cpu().view(torch.uint8)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_raw(a), _raw(b))


class _Sums:
    """Replica sums of one BatchNorm over C channels ([nrep][S] fp64, the derived sums in front, room for the consumer's own
    sums behind them: the replica stride is process-wide) and everything else the two finalize kernels read."""

    def __init__(self, kind, C, nrep, count, extra, seed):
        g = torch.Generator().manual_seed(seed)
        self.kind, self.C, self.nrep, self.count, self.S = kind, C, nrep, float(count), 2 * C + extra
        share = torch.rand(nrep, C, generator=g, dtype=torch.float64) + 0.1
        share = share / share.sum(0)
        buf = torch.zeros(nrep, self.S, dtype=torch.float64)
        if kind == 1:
            mean = torch.randn(C, generator=g, dtype=torch.float64) * 0.5
            var = torch.rand(C, generator=g, dtype=torch.float64) + 0.1
            var[0] = -1e-9                   # a variance the one-pass formula leaves below zero: clamped
            s1, s2 = mean * count, (var + mean * mean) * count
        else:
            s1 = torch.randn(C, generator=g, dtype=torch.float64) * 3
            s2 = torch.randn(C, generator=g, dtype=torch.float64) * 3
        buf[:, :C], buf[:, C:2 * C] = share * s1, share * s2
        self.buf = buf.cuda()
        f32 = lambda t: t.float().cuda()
        self.gamma = f32(torch.rand(C, generator=g) + 0.5)
        self.beta = f32(torch.randn(C, generator=g) * 0.3)
        self.mean = f32(torch.randn(C, generator=g) * 0.2)
        self.invstd = f32(torch.rand(C, generator=g) + 0.5)
        self.rm0, self.rv0 = f32(torch.randn(C, generator=g)), f32(torch.rand(C, generator=g) + 0.5)

    def own(self, n):
        """The consumer's own sums: 2 n doubles of replica 0 behind the derived ones."""
        assert 2 * self.C + 2 * n <= self.S
        return self.buf[0, 2 * self.C:2 * self.C + 2 * n]

    def fresh(self):
        nan = lambda: torch.full((self.C,), float('nan'), device='cuda')
        o = dict(o0=nan(), o1=nan(), o2=nan(), o3=nan(), o4=nan())
        if self.kind == 1:
            o.update(rm=self.rm0.clone(), rv=self.rv0.clone(), nbt=torch.full((1,), 41, dtype=torch.int64, device='cuda'))
        self.buf[:, 2 * self.C:].zero_()
        return o

    def finalize(self, o):
        from torchdet3d import _native as N
        if self.kind == 1:
            N.call('t3d_bn_finalize', N.ptr(self.buf), self.C, self.count, N.ptr(self.gamma), N.ptr(self.beta), N.ptr(o['rm']),
                   N.ptr(o['rv']), N.ptr(o['nbt']), MOM, EPS, N.ptr(o['o0']), N.ptr(o['o1']), N.ptr(o['o2']), N.ptr(o['o3']), N.stream())
        else:
            N.call('t3d_bn_bwd_finalize', N.ptr(self.buf), self.C, self.count, N.ptr(self.gamma), N.ptr(self.mean),
                   N.ptr(self.invstd), N.ptr(o['o0']), N.ptr(o['o1']), N.ptr(o['o2']), N.ptr(o['o3']), N.ptr(o['o4']), N.stream())

    def request(self, o):
        from torchdet3d import _native as N
        f = N.BnFold()
        f.kind, f.C, f.nrep, f.rstride, f.count = self.kind, self.C, self.nrep, self.S, self.count
        f.stats, f.gamma = N.ptr(self.buf), N.ptr(self.gamma)
        f.o0, f.o1, f.o2, f.o3 = (N.ptr(o[k]) for k in ('o0', 'o1', 'o2', 'o3'))
        if self.kind == 1:
            f.beta, f.rm, f.rv, f.nbt, f.momentum, f.eps = N.ptr(self.beta), N.ptr(o['rm']), N.ptr(o['rv']), N.ptr(o['nbt']), MOM, EPS
        else:
            f.mean, f.invstd, f.o4 = N.ptr(self.mean), N.ptr(self.invstd), N.ptr(o['o4'])
        desc = torch.frombuffer(bytearray(bytes(f)), dtype=torch.uint8).cuda()
        N.call('t3d_fold_request', N.ptr(desc), N.ptr(o['o0']))
        return desc


def _both_ways(sums, consumer, published=True):
    """consumer(o) launches the kernel under test reading the coefficient arrays o['o0'] .. and returns its output tensors.
    Runs it behind the standalone finalize and with the finalize requested of the launch itself; everything byte-equal."""
    from torchdet3d import _native as N
    res = {}
    N.call('t3d_set_reduction_replicas', sums.nrep, sums.S)
    try:
        for lazy in (False, True):
            o = sums.fresh()
            keep = sums.request(o) if lazy else sums.finalize(o)
            outs = consumer(o)
            assert N.lib().t3d_fold_pending() == 0, 'the launch left the finalize request unserved'
            torch.cuda.synchronize()
            res[lazy] = ({k: v.clone() for k, v in o.items()}, [t.clone() for t in outs] + [sums.buf[:, 2 * sums.C:].clone()])
            del keep
    finally:
        N.lib().t3d_fold_pending()
        N.call('t3d_set_reduction_replicas', 1, 0)
    names = (('o0', 'o1', 'o2', 'o3', 'rm', 'rv', 'nbt') if sums.kind == 1 else ('o0', 'o1', 'o2', 'o3', 'o4')) if published else ()
    for k in names:
        a, b = res[False][0][k], res[True][0][k]
        assert not torch.isnan(a.float()).any(), k
        assert _same(a, b), f'published {k} differs from the standalone finalize'
    if sums.kind == 1 and published:
        assert int(res[True][0]['nbt'].item()) == 42
    assert len(res[False][1]) == len(res[True][1])
    for i, (a, b) in enumerate(zip(res[False][1], res[True][1])):
        assert torch.isfinite(a.double()).all(), i
        assert _same(a, b), f'output {i} differs from finalize + plain launch'


def _bf(shape, g, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(BF).cuda()


def _frag(wd):
    from torchdet3d import _native as N
    r, c = wd.shape
    out = torch.zeros(N.lib().t3d_pwconv_frag_bytes(r, c) // 2, device='cuda', dtype=BF)
    N.call('t3d_pwconv_pack_frag', N.ptr(wd), N.ptr(out), r, c, N.stream())
    return out


class _forced_pw:
    def __init__(self, route):
        self.route = route

    def __enter__(self):
        from torchdet3d import _native as N
        N.call('t3d_pwconv_force_route', self.route)

    def __exit__(self, *a):
        from torchdet3d import _native as N
        N.call('t3d_pwconv_force_route', N.PW_AUTO)


# ---- consumers ---------------------------------------------------------------------------------------------------------------
def _pw_fwd(sums, B, HW, K, Nn, seed, route='stream', mat=False):
    """t3d_pwconv_fwd / _fwd_mat, K -> Nn, the operand's BatchNorm (K channels, kind 1) derived; own statistics on."""
    from torchdet3d import _native as N
    g = torch.Generator().manual_seed(seed)
    M = B * HW
    x, w, r = _bf((M, K), g), _bf((Nn, K), g, K ** -0.5), _bf((M, K), g)
    deep = route == 'deep'
    code, wv = (N.BF16 | N.W_FRAG, _frag(w)) if deep else (N.BF16, w)

    def run(o):
        pro = N.prologue(o['o0'], o['o1'], None, 'relu6', False)
        y = torch.empty(M, Nn, device='cuda', dtype=BF)
        with _forced_pw(N.PW_DEEP if deep else N.PW_STREAM):
            if mat:
                z = torch.empty(M, K, device='cuda', dtype=BF)
                N.call('t3d_pwconv_fwd_mat', code, N.ptr(x), pro, N.ptr(r), N.ptr(z), N.ptr(wv), N.ptr(y), N.ptr(sums.own(Nn)),
                       M, HW, K, Nn, N.stream())
                return [z, y]
            N.call('t3d_pwconv_fwd', code, N.ptr(x), pro, N.ptr(wv), None, N.ptr(y), N.ptr(sums.own(Nn)), M, HW, K, Nn, N.stream())
        return [y]
    return run


def _pw_dgrad(sums, B, HW, K, Nn, seed, route='stream'):
    """t3d_pwconv_dgrad of a layer K -> Nn: contraction over the Nn channels whose BatchNorm-backward coefficients (kind 2) are
    derived; activation derivative and own sums on."""
    from torchdet3d import _native as N
    g = torch.Generator().manual_seed(seed)
    M = B * HW
    dz, y, xraw = _bf((M, Nn), g), _bf((M, Nn), g), _bf((M, K), g)
    wt = _bf((K, Nn), g, Nn ** -0.5)
    sc, sh = (torch.rand(K, generator=g) + 0.5).cuda(), (torch.randn(K, generator=g) * 0.3).cuda()
    deep = route == 'deep'
    code, wv = (N.BF16 | N.W_FRAG, _frag(wt)) if deep else (N.BF16, wt)

    def run(o):
        bb = N.bnbwd(o['o0'], o['o1'], o['o2'], False)
        pin = N.prologue(sc, sh, None, 'relu6', False)
        dx = torch.empty(M, K, device='cuda', dtype=BF)
        with _forced_pw(N.PW_DEEP if deep else N.PW_STREAM):
            N.call('t3d_pwconv_dgrad', code, N.ptr(dz), N.ptr(y), bb, N.ptr(wv), N.ptr(xraw), pin, None, N.ptr(dx),
                   N.ptr(sums.own(K)), None, M, HW, K, Nn, N.stream())
        return [dx]
    return run


# ---- derived and published coefficients: every replica count x channel count, both kinds ----------------------------------------
@pytest.mark.parametrize('C', [8, 24, 72, 200])
@pytest.mark.parametrize('nrep', [1, 2, 3, 8, 16])
@pytest.mark.parametrize('kind', [1, 2])
def test_derived_and_published_coefficients(kind, nrep, C):
    B, HW, other = 2, 63, 16
    sums = _Sums(kind, C, nrep, B * HW, 2 * other, 1000 * kind + 10 * nrep + C)
    consumer = _pw_fwd(sums, B, HW, C, other, C + nrep) if kind == 1 else _pw_dgrad(sums, B, HW, other, C, C + nrep)
    _both_ways(sums, consumer)


# ---- one case per kernel family with a derive prologue --------------------------------------------------------------------------
PLANES = [((9, 7), 3), ((4, 4), 16)]      # plane, replica count


@pytest.mark.parametrize('plane,nrep', PLANES)
@pytest.mark.parametrize('K,Nn', [(24, 72), (72, 24), (200, 40)])
@pytest.mark.parametrize('mat', [False, True])
def test_pwconv_fwd_serves_the_request(plane, nrep, K, Nn, mat):
    HW = plane[0] * plane[1]
    sums = _Sums(1, K, nrep, 2 * HW, 2 * Nn, K + Nn)
    _both_ways(sums, _pw_fwd(sums, 2, HW, K, Nn, K + HW, mat=mat))


@pytest.mark.parametrize('plane,nrep', PLANES)
@pytest.mark.parametrize('K,Nn', [(24, 72), (72, 24), (40, 200)])
def test_pwconv_dgrad_stream_serves_the_request(plane, nrep, K, Nn):
    HW = plane[0] * plane[1]
    sums = _Sums(2, Nn, nrep, 2 * HW, 2 * K, K + Nn + 1)
    _both_ways(sums, _pw_dgrad(sums, 2, HW, K, Nn, K + HW))


@pytest.mark.parametrize('plane,nrep', PLANES)
def test_pwconv_deep_route_serves_the_request(plane, nrep):
    """The deep-contraction kernel takes contractions of 512 channels and more only (t3d_pwconv_wants_frag), so the 200 -> 40
    layer above runs through the streaming kernel; its smallest shape is checked here: 520 -> 104, forward and data gradient."""
    from torchdet3d import _native as N
    HW = plane[0] * plane[1]
    assert N.lib().t3d_pwconv_wants_frag(520, 104) == 1 and N.lib().t3d_pwconv_wants_frag(200, 40) == 0
    sums = _Sums(1, 520, nrep, 2 * HW, 2 * 104, 520)
    _both_ways(sums, _pw_fwd(sums, 2, HW, 520, 104, HW, route='deep'))
    sums = _Sums(2, 520, nrep, 2 * HW, 2 * 104, 521)
    _both_ways(sums, _pw_dgrad(sums, 2, HW, 104, 520, HW + 1, route='deep'))


@pytest.mark.parametrize('plane,nrep', PLANES)
@pytest.mark.parametrize('K,Nn', [(24, 72), (72, 24)])
def test_pwconv_wgrad_serves_the_request(plane, nrep, K, Nn):
    """The weight gradient derives without publishing (include/t3d.h): its output alone is compared."""
    from torchdet3d import _native as N
    HW = plane[0] * plane[1]
    M = 2 * HW
    g = torch.Generator().manual_seed(K + HW)
    dz, y, x = _bf((M, Nn), g), _bf((M, Nn), g), _bf((M, K), g)
    sc, sh = (torch.rand(K, generator=g) + 0.5).cuda(), (torch.randn(K, generator=g) * 0.3).cuda()
    sums = _Sums(2, Nn, nrep, M, 0, K + Nn + 2)

    def run(o):
        bb = N.bnbwd(o['o0'], o['o1'], o['o2'], False)
        dw = torch.zeros(Nn, K, device='cuda')
        N.call('t3d_pwconv_wgrad', N.BF16, N.ptr(dz), N.ptr(y), bb, N.ptr(x), N.prologue(sc, sh, None, 'relu6', False), N.ptr(dw),
               M, HW, K, Nn, N.stream())
        return [dw]
    assert N.lib().t3d_pwconv_route(N.PW_OP_WGRAD, N.BF16, 0, 0, 0, 0, 0, 0, 1, N.ACT['relu6'], 0, M, HW, K, Nn) == N.PW_TR
    _both_ways(sums, run, published=False)


@pytest.mark.parametrize('plane,nrep', PLANES)
@pytest.mark.parametrize('K,Nn', [(24, 72), (72, 24)])
def test_pwconv_yfree_prep_serves_the_request(plane, nrep, K, Nn):
    from torchdet3d import _native as N
    g = torch.Generator().manual_seed(K + Nn + 3)
    wt = _bf((K, Nn), g, Nn ** -0.5)
    NP, KP = (Nn + 31) // 32 * 32, (K + 31) // 32 * 32
    sums = _Sums(2, Nn, nrep, 2 * plane[0] * plane[1], 0, K + Nn + 4)

    def run(o):
        bb = N.bnbwd(o['o0'], o['o1'], o['o2'], False)
        wcat, cvec = torch.zeros(K, NP + KP, device='cuda', dtype=BF), torch.zeros(K, device='cuda')
        N.call('t3d_pwconv_yfree_prep', N.ptr(wt), bb, N.ptr(wcat), N.ptr(cvec), K, Nn, N.stream())
        return [wcat, cvec]
    _both_ways(sums, run)


@pytest.mark.parametrize('plane,nrep', PLANES)
def test_bn_apply_serves_the_request(plane, nrep):
    from torchdet3d import _native as N
    C, M = 72, 2 * plane[0] * plane[1]
    g = torch.Generator().manual_seed(M)
    y, r = _bf((M, C), g), _bf((M, C), g)
    sums = _Sums(1, C, nrep, M, 0, M + 5)

    def run(o):
        z = torch.empty(M, C, device='cuda', dtype=BF)
        N.call('t3d_bn_apply', N.BF16, N.ptr(y), N.prologue(o['o0'], o['o1'], None, 'relu6', False), N.ptr(r), N.ptr(z), M, C, N.stream())
        return [z]
    _both_ways(sums, run)


@pytest.mark.parametrize('plane,nrep', PLANES)
def test_dwconv_fwd_serves_the_request(plane, nrep):
    from torchdet3d import _native as N
    B, (H, W), C = 2, plane, 72
    g = torch.Generator().manual_seed(H * W)
    x = _bf((B, H, W, C), g)
    w = (torch.randn(C, 9, generator=g) * 0.3).cuda()
    sums = _Sums(1, C, nrep, B * H * W, 2 * C, H * W + 6)

    def run(o):
        y = torch.empty(B, H, W, C, device='cuda', dtype=BF)
        N.call('t3d_dwconv_fwd', N.BF16, N.ptr(x), N.prologue(o['o0'], o['o1'], None, 'relu6', False), N.ptr(w), N.ptr(y),
               N.ptr(sums.own(C)), None, B, H, W, C, 3, 1, N.stream())
        return [y]
    assert N.lib().t3d_dwconv_route(0, N.BF16, 0, 0, B, H, W, C, 3, 1) == N.DW_ROW3
    _both_ways(sums, run)


@pytest.mark.parametrize('plane,nrep', PLANES)
@pytest.mark.parametrize('s', [1, 2])
def test_dwconv_bwd_serves_the_request(plane, nrep, s):
    from torchdet3d import _native as N
    B, (H, W), C = 2, plane, 72
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    g = torch.Generator().manual_seed(H * W + s)
    x, dz, y = _bf((B, H, W, C), g), _bf((B, Ho, Wo, C), g, 0.1), _bf((B, Ho, Wo, C), g)
    w = (torch.randn(C, 9, generator=g) * 0.3).cuda()
    sc, sh = (torch.rand(C, generator=g) + 0.5).cuda(), (torch.randn(C, generator=g) * 0.2).cuda()
    sums = _Sums(2, C, nrep, B * Ho * Wo, 2 * C, H * W + 7)
    SLOTS = 64
    used = torch.zeros(1, dtype=torch.int32, device='cuda')

    def run(o):
        bb = N.bnbwd(o['o0'], o['o1'], o['o2'], False)
        dx = torch.empty(B, H, W, C, device='cuda', dtype=BF)
        dw = torch.zeros(SLOTS, C, 9, device='cuda')        # one weight-gradient slot per workgroup: stores, no atomics
        N.call('t3d_dwconv_bwd', N.BF16, N.ptr(dz), N.ptr(y), bb, N.ptr(w), N.ptr(x), N.prologue(sc, sh, None, 'relu6', False), None,
               N.ptr(dx), N.ptr(sums.own(C)), N.ptr(dw), B, H, W, C, 3, s, N.stream())
        return [dx, dw]
    assert N.lib().t3d_dwconv_route(1, N.BF16, 0, 0, B, H, W, C, 3, s) == N.DW_ROW3
    N.call('t3d_set_dw_slots', SLOTS, N.ptr(used))
    try:
        _both_ways(sums, run)
    finally:
        N.call('t3d_set_dw_slots', 0, None)
    assert 1 <= int(used.item()) <= SLOTS


# ---- the statistics tail of the streaming kernel against recorded sums ----------------------------------------------------------
TAIL_B, TAIL_HW, TAIL_DEPTH = 3, 25, 24


def _pattern(rows, cols, a, b, m, div):
    """Integer pattern in [-m/2, m/2] / div: exact in bf16 for m <= 256."""
    i, j = np.meshgrid(np.arange(rows, dtype=np.int64), np.arange(cols, dtype=np.int64), indexing='ij')
    return torch.from_numpy((((i * a + j * b + i * j) % (m + 1)) - m // 2).astype(np.float32) / div)


def _tail_sums(op, nout, nrep):
    """[nrep][2 nout] fp64: the sums t3d_pwconv_fwd (sum y, sum y^2) or t3d_pwconv_dgrad (sum dx, sum dx . x_raw) leaves for
    B = 3 @ 5x5 pixels, a contraction over 24 channels and `nout` output channels, through the streaming kernel."""
    from torchdet3d import _native as N
    M, D = TAIL_B * TAIL_HW, TAIL_DEPTH
    dev = lambda t: t.to(BF).cuda()
    x = dev(_pattern(M, D, 7919, 104729, 256, 64.0))
    w = dev(_pattern(nout, D, 31, 17, 128, 256.0))
    c0 = (_pattern(1, D, 5, 3, 64, 64.0)[0] + 1.25).cuda()
    c1 = (_pattern(1, D, 11, 7, 64, 128.0)[0]).cuda()
    c2 = (_pattern(1, D, 13, 5, 64, 256.0)[0]).cuda()
    st = torch.zeros(nrep, 2 * nout, device='cuda', dtype=torch.float64)
    out = torch.empty(M, nout, device='cuda', dtype=BF)
    N.call('t3d_set_reduction_replicas', nrep, 2 * nout)
    try:
        with _forced_pw(N.PW_STREAM):
            if op == 'fwd':
                N.call('t3d_pwconv_fwd', N.BF16, N.ptr(x), N.prologue(c0, c1, None, 'relu6', False), N.ptr(w), None, N.ptr(out), N.ptr(st),
                       M, TAIL_HW, D, nout, N.stream())
            else:
                y = dev(_pattern(M, D, 101, 977, 256, 64.0))
                xraw = dev(_pattern(M, nout, 389, 53, 256, 64.0))
                wt = w                                            # [nout][D]: the transposed copy of a D x nout layer's weights
                e0 = (_pattern(1, nout, 3, 7, 64, 64.0)[0] + 1.5).cuda()
                e1 = (_pattern(1, nout, 9, 2, 64, 32.0)[0]).cuda()
                N.call('t3d_pwconv_dgrad', N.BF16, N.ptr(x), N.ptr(y), N.bnbwd(c0, c1, c2, False), N.ptr(wt), N.ptr(xraw),
                       N.prologue(e0, e1, None, 'relu6', False), None, N.ptr(out), N.ptr(st), None, M, TAIL_HW, nout, D, N.stream())
    finally:
        N.call('t3d_set_reduction_replicas', 1, 0)
    torch.cuda.synchronize()
    return st.cpu().numpy()


TAIL_CASES = [(op, nout, nrep) for op in ('fwd', 'dgrad') for nout in (16, 40, 96) for nrep in (1, 4)]


@pytest.mark.parametrize('op,nout,nrep', TAIL_CASES)
def test_streaming_kernel_sums_equal_the_recorded_ones(op, nout, nrep):
    """nout = 16 and 40 leave a 32-channel block of the tail partly past the last channel."""
    want = np.load(GOLDEN)[f'{op}_{nout}_{nrep}']
    got = _tail_sums(op, nout, nrep)
    assert np.abs(want).sum() > 0 and (want[1:] == 0).all()       # (one workgroup: everything lands in replica 0)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float64
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))


if __name__ == '__main__':
    if '--write-golden' in sys.argv:
        sys.path[:0] = [os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), '3d-object-detection.pytorch_amd')]
        out = sys.argv[sys.argv.index('--write-golden') + 1] if len(sys.argv) > sys.argv.index('--write-golden') + 1 else GOLDEN
        np.savez(out, **{f'{op}_{nout}_{nrep}': _tail_sums(op, nout, nrep) for op, nout, nrep in TAIL_CASES})
        print('wrote', out)
