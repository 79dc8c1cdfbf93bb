"""CPU: the options of the device crop cache (dataloaders/gpu_loader.py, builders/loader_builder.py) -- `cfg.data.cache`
is nothing or 'device', the arena is checked against `cfg.data.cache_max_gb` when the loader is built, without a GPU -- and
the C ABI of `t3d_augment_resized_u8` (header, ctypes table, unchanged record layout)."""
import os

import pytest

import augment_ref as R
from conftest import ROOT


@pytest.fixture(scope='module')
def root(tmp_path_factory):
    return R.write_dataset(str(tmp_path_factory.mktemp('objectron')), seed=3)


def _cfg(root, **data):
    from torchdet3d.utils import AttrDict
    tr, te = R.default_pipelines((224, 224))
    d = dict(root=root, resize=(224, 224), train_batch_size=4, val_batch_size=3, num_workers=0, category_list='all',
             normalization=R.NORMALIZATION)
    d.update(data)
    return AttrDict(dict(data=d, utils=dict(random_seeds=5), model=dict(num_classes=9), train_data_pipeline=tr,
                         test_data_pipeline=te))


def test_cache_absent_or_falsy_is_the_uncached_loader(root):
    from torchdet3d.builders import build_loader
    for extra in ({}, dict(cache=None), dict(cache=False), dict(cache='')):
        for ld in build_loader(_cfg(root, **extra)):
            assert ld.cache is None
            assert not any(k in vars(ld) for k in ('_arena', '_c_kp', '_c_desc', '_c_cats'))
            with pytest.raises(RuntimeError, match='cache'):
                ld.fill_cache()


def test_unknown_cache_value_raises(root):
    from torchdet3d.builders import build_loader
    for bad in ('host', 'disk', True, 1):
        with pytest.raises(ValueError, match='data.cache'):
            build_loader(_cfg(root, cache=bad))


def test_device_cache_is_accepted_and_nothing_is_filled_at_construction(root):
    from torchdet3d.builders import build_loader
    train, val, test = build_loader(_cfg(root, cache='device'))
    for ld in (train, val, test):
        assert ld.cache == 'device' and ld._arena is None
    # what existing callers read keeps its meaning
    assert len(train) == len(train.dataset) // 4 and len(val) == -(-len(val.dataset) // 3) and len(test) == len(test.dataset)
    train.sampler.set_epoch(2)
    assert train.sampler.epoch == 2 and train.loader.batch_sampler is not None and train.pipeline.is_random


def test_budget_is_checked_at_construction_and_names_both_figures(root):
    from torchdet3d.builders import build_loader
    from torchdet3d.dataloaders import GpuAugmentLoader, Objectron, build_augmentations
    ds = Objectron(root, mode='train')
    need = len(ds) * 224 * 224 * 3
    with pytest.raises(ValueError) as e:
        build_loader(_cfg(root, cache='device', cache_max_gb=0.001))
    msg = str(e.value)
    assert str(need) in msg and '0.001' in msg and str(int(0.001 * 2 ** 30)) in msg
    # the budget is the arena's size exactly: one byte less does not fit, the size itself does
    pipe = build_augmentations(_cfg(root))[0]
    GpuAugmentLoader(ds, pipe, 4, cache='device', cache_max_gb=need / 2 ** 30)
    with pytest.raises(ValueError, match=str(need)):
        GpuAugmentLoader(ds, pipe, 4, cache='device', cache_max_gb=(need - 1) / 2 ** 30)
    # the default budget is 32 GB
    assert 'cache_max_gb = 32 ' in _budget_message(ds, pipe)


def _budget_message(ds, pipe):
    from torchdet3d.dataloaders import GpuAugmentLoader

    class Huge:
        def __len__(self):
            return (32 * 2 ** 30) // (224 * 224 * 3) + 1

    with pytest.raises(ValueError) as e:
        GpuAugmentLoader(Huge(), pipe, 4, sampler=range(4), cache='device')
    return str(e.value)


def test_symbol_in_the_header_and_the_ctypes_table_record_unchanged():
    from torchdet3d import _native as N
    from torchdet3d.dataloaders.objectron import AUG_SAMPLE_DTYPE
    src = open(os.path.join(ROOT, 'include', 't3d.h')).read()
    # (the declaration against the binding's types: tests/test_abi.py)
    assert N.SIGNATURES['t3d_augment_resized_u8'] == N.SIGNATURES['t3d_augment_crops_u8']
    assert 'objectron_main.py:51-96' in src[src.index('The same augmentations over crops'):src.index('int t3d_augment_resized_u8')]
    assert AUG_SAMPLE_DTYPE.itemsize == 80 and AUG_SAMPLE_DTYPE.names == ('offset', 'h', 'w', 'flags', 'alpha', 'beta255',
                                                                          'reserved', 'm')
