"""CPU checks behind tests/test_gpu_detector_train.py: the conditioning of the gradient case, the restatement against plain
autograd of the oracle's own forward, and the flat layout `DetectorTrainer` relies on.

Conditioning.  The GPU test bounds every gradient tensor by 4 x the float32-against-float64 spread of the restatement
(tests/ssd_backbone_ref.py: `spreads`, scale floored at 1e-3 of the largest gradient).  That only means something where the
spread is small: a ReLU6 kink that flips between float32 and float64 moves a gradient by 5e-2 .. 2e-1 of its size (2 x 64 x 96,
3 x 96 x 96, 2 x 128 x 160, 4 x 128 x 128 all do).  The case used -- mobilenetv2, make_state_dict(seed 0), make_inputs(2, 96,
128) -- has no such flip: worst tensor features.1.conv.5.bias 2.9e-4, median 1.7e-5; the cap asserted here is 1e-3.  The
float32 run's summation order, and with it the flips, depends on torch's CPU thread count: the restatement pins it
(ssd_backbone_ref.REF_THREADS), so the figures are the same on every host and anywhere in a suite whose other tests change it.
"""
import numpy as np
import torch

import ssd_backbone_ref as R

CAP = 1e-3


def _worst(spread):
    return max((v[0], k) for k, v in spread.items())


def test_the_gradient_case_is_well_conditioned():
    for zero in ((), (17,), (13,)):
        c = R.case(zero)
        worst, key = _worst(c['spread'])
        med = float(np.median([v[0] for v in c['spread'].values()]))
        print(f'zero cotangent at {zero}: worst spread {worst:.3e} ({key}), median {med:.3e}; taps '
              + ', '.join(f'{k}: {v[0]:.3e}' for k, v in c['tap_spread'].items()))
        assert set(c['spread']) == set(R.trained_keys(c['sd']))
        assert worst <= CAP, (zero, key, worst)
        assert all(np.isfinite(v).all() for v in c['r64']['grads'].values())


def test_the_restatement_does_not_depend_on_the_callers_thread_count():
    n = torch.get_num_threads()
    ref = R.case()['r32']['grads']['features.11.conv.4.bias'].copy()
    try:
        torch.set_num_threads(1)
        R.case.cache_clear()
        again = R.case()['r32']['grads']['features.11.conv.4.bias']
        assert torch.get_num_threads() == 1
    finally:
        torch.set_num_threads(n)
    np.testing.assert_array_equal(ref, again)


def test_cotangents_are_storage_values_and_seeded():
    dims = R.tap_dims(2, 96, 128)
    assert dims == {13: (2, 6, 8, 96), 17: (2, 3, 4, 320)}
    assert R.tap_dims(2, 300, 300) == {13: (2, 19, 19, 96), 17: (2, 10, 10, 320)}
    a, b = R.cotangents(dims, 0, True), R.cotangents(dims, 0, True)
    for k in dims:
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], a[k].to(torch.bfloat16).float())
        assert a[k].shape == (dims[k][0] * dims[k][1] * dims[k][2], dims[k][3])
    assert not R.cotangents(dims, 0, False, zero=(17,))[17].any()


def test_restatement_is_the_oracles_forward_cut_at_the_taps():
    """The taps are the oracle's `extract_features` taps, the running statistics move exactly as the oracle moves them, and
    nothing behind features.17 is touched."""
    from oracle.model import extract_features
    from oracle.specs import arch
    c = R.case()
    sd = {k: v.clone() for k, v in c['sd'].items()}
    all_taps = {}
    extract_features(sd, arch(R.NAME), c['imgs'], True, all_taps)
    r32 = c['r32']
    for k in R.TAPS:
        np.testing.assert_array_equal(R.rows(all_taps[f'features.{k}']).double().numpy(), r32['taps'][k])
    for k, v in r32['buffers'].items():
        np.testing.assert_array_equal(sd[k].double().numpy(), v)
        if k.endswith('num_batches_tracked'):
            assert int(v) == int(c['sd'][k]) + 1
    assert not any(k.startswith(('conv.', 'classifier.', 'cls_fc.', 'regressors.')) for k in r32['buffers'])
    # a zero cotangent at the deepest tap: nothing of features.14 .. 17 has a gradient
    z = R.case((17,))
    for k, v in z['r64']['grads'].items():
        if int(k.split('.')[1]) >= 14:
            assert not v.any(), k
        elif k.endswith('weight') and v.ndim == 4:
            assert v.any(), k


def test_trained_prefix_of_the_flat_layout():
    """The stem and features.* are a contiguous prefix of the engine's flat parameter buffer, ending where conv.0.weight
    starts; everything the detector does not use lies behind it."""
    from torchdet3d.models.engine import Net
    net = Net('mobilenetv2', 9, 'cpu', torch.float32)
    n = net.offsets['conv.0.weight'][0]
    assert n == net.offsets[net.arch.keys.last_w][0] and n % 4 == 0 and 0 < n < net.nparams
    for k, (o, m) in net.offsets.items():
        inside = k.startswith('features.')
        assert (o + m <= n) if inside else (o >= n), k
    assert set(k for k in net.p if k.startswith('features.')) == set(R.trained_keys(R.case()['sd']))
    ends = sorted((o, o + (m + 3) // 4 * 4) for k, (o, m) in net.offsets.items() if k.startswith('features.'))
    assert ends[0][0] == 0 and ends[-1][1] == n and all(a[1] == b[0] for a, b in zip(ends, ends[1:]))


def test_sgd_restatement_matches_torch():
    g = torch.Generator().manual_seed(3)
    p0, gr = torch.randn(50, generator=g, dtype=torch.float64), torch.randn(50, generator=g, dtype=torch.float64)
    p = p0.clone().requires_grad_(True)
    opt = torch.optim.SGD([p], lr=0.05, momentum=0.9, weight_decay=5e-4)
    want, buf = p0.numpy(), np.zeros(50)
    for _ in range(3):
        p.grad = gr.clone()
        opt.step()
        want, buf = R.sgd_step(want, gr.numpy(), buf, 0.05)
    np.testing.assert_allclose(p.detach().numpy(), want, rtol=1e-13, atol=1e-15)
