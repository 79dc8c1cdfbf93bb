"""CPU checks of the joined frame pipeline (torchdet3d/utils/pipeline.py, csrc/pipeline.hip): `FramePipeline` is part of the
public surface and refuses to run without a GPU, and `SSD300.merge_classes` is the merge `SSD300.detect` used to do inline.
(That the three joint kernels and t3d_track_step are declared, bound and recordable into a plan: tests/test_abi.py.)"""
import numpy as np
import pytest
import torch


def test_frame_pipeline_is_exported_and_needs_a_gpu():
    import torchdet3d.utils as U
    from torchdet3d.utils import FramePipeline
    assert U.FramePipeline is FramePipeline
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            FramePipeline(None, None, None)


def test_merge_classes_is_the_detectors_inline_merge():
    from torchdet3d.models.ssd import INPUT_SIZE, SSD300
    rng = np.random.default_rng(0)
    nc, K, max_per_img = 3, 5, 7
    out = rng.uniform(0, 300, (nc, K, 6)).astype(np.float32)
    out[:, :, 4] = rng.uniform(0.02, 1, (nc, K)).astype(np.float32)
    out[1, 0, 4] = out[0, 1, 4]                                       # equal scores across classes: class order decides
    out[2, 1, 4] = out[0, 1, 4]
    for c in range(nc):
        out[c, :, 5] = c
    cnt = np.array([4, 2, 5], np.int32)
    keep = out.copy()
    got = SSD300.merge_classes(out, cnt, max_per_img)
    assert np.array_equal(out, keep), 'the helper works on a copy'
    # the code as it stood inline in SSD300.detect
    rows = np.concatenate([keep[c, :cnt[c]] for c in range(nc)]) if cnt.sum() else np.zeros((0, 6), np.float32)
    order = np.argsort(-rows[:, 4], kind='stable')[:max_per_img]
    rows = rows[order]
    rows[:, :4] /= INPUT_SIZE
    assert got.dtype == np.float32 and got.shape == (7, 6)
    assert np.array_equal(got, rows)
    tied = [i for i in range(len(got)) if got[i, 4] == keep[0, 1, 4]]
    assert [int(got[i, 5]) for i in tied] == [0, 1, 2]
    empty = SSD300.merge_classes(keep, np.zeros(nc, np.int32), max_per_img)
    assert empty.shape == (0, 6) and empty.dtype == np.float32
