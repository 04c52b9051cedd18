"""
The tests' wide-index build of the library (``_build.WIDE_LIB_PATH``,
``-DREMAP_ROWPASS_WIDE_INDEX``): it exists after ``build()``, carries the
product's ABI plus the mark ``remap_rowpass_wide_index``, and its five row
passes answer as the product's do before anything touches a device.  What it
computes is checked on the GPU (tests/test_gpu_wide_index.py).
"""
import ctypes
import os

import pytest

from helpers import REPO

MARK = 'remap_rowpass_wide_index'
ENTRIES = (('remap_limit_rows', '_LimitArgs'),
           ('remap_apply_sgs', '_SgsArgs'),
           ('remap_apply_vector', '_VectorArgs'),
           ('remap_apply_levels', '_LevelsArgs'),
           ('remap_apply_layers', '_LayersArgs'))


@pytest.fixture(scope='module')
def wide():
    from pyremap_amd import _build, engine
    engine.load_library()           # (torch's HIP runtime first, as always)
    assert os.path.exists(_build.WIDE_LIB_PATH), \
        f'{_build.WIDE_LIB_PATH} is missing: build() makes it'
    return engine.open_library(_build.WIDE_LIB_PATH)


def test_the_wide_library_is_a_test_artefact_beside_the_product():
    from pyremap_amd import _build, engine
    assert _build.WIDE_LIB_PATH == os.path.join(
        REPO, 'pyremap_amd', '_lib', 'libremap_hip_wideindex.so')
    assert _build.WIDE_LIB_PATH != engine.library_path()
    assert _build.ROWPASS_SOURCES == [
        'remap_limit.hip', 'remap_sgs.hip', 'remap_vector.hip',
        'remap_levels.hip', 'remap_layers.hip']
    assert set(_build.ROWPASS_SOURCES) < set(_build.SOURCES)
    assert len(_build.SOURCES) - len(_build.ROWPASS_SOURCES) == 13
    # one switch, in one place, and a mark no header declares
    csrc = {name: open(os.path.join(_build.CSRC, name)).read()
            for name in os.listdir(_build.CSRC)}
    users = sorted(name for name, text in csrc.items()
                   if 'REMAP_ROWPASS_WIDE_INDEX' in text)
    assert users == ['libremap_hip.map', 'remap_limit.hip', 'rowpass.h']
    header = open(os.path.join(REPO, 'include', 'remap_hip.h')).read()
    assert MARK not in header and MARK not in engine.EXPORTS
    assert MARK in csrc['libremap_hip.map']
    # the package itself never loads it
    for root, _, files in os.walk(os.path.join(REPO, 'pyremap_amd')):
        for name in files:
            if name.endswith('.py') and name != '_build.py':
                text = open(os.path.join(root, name)).read()
                assert 'wideindex' not in text and \
                    'build_wide_index_library' not in text, name


def test_exports_and_the_mark(wide):
    from pyremap_amd import engine
    product = engine.load_library()
    assert wide is not product
    for name in engine.EXPORTS:
        assert hasattr(wide, name), name
    assert hasattr(wide, MARK)
    fn = getattr(wide, MARK)
    fn.restype, fn.argtypes = ctypes.c_int, []
    assert fn() == 1
    assert not hasattr(product, MARK)
    assert wide.remap_abi_version() == product.remap_abi_version() == \
        engine.ABI_VERSION
    assert wide.remap_arch() == product.remap_arch()
    # opening the second library leaves the package's own in place
    assert engine.load_library() is product


@pytest.mark.parametrize('entry, struct', ENTRIES)
def test_row_passes_answer_before_any_device(wide, entry, struct):
    """An empty launch is REMAP_OK and NULL args are REMAP_ERR_ARG with a
    message, as in the product: both return in front of the dispatch."""
    from pyremap_amd import engine
    product = engine.load_library()
    for lib in (wide, product):
        call = getattr(lib, entry)
        assert call(None, None) == -1
        msg = lib.remap_last_error()
        assert entry.encode() in msg and b'NULL args' in msg
        args = getattr(engine, struct)()
        args.A.n_rows, args.A.n_cols = 4, 6
        args.row_begin, args.row_end = 0, 4
        args.n_batch, args.k_inner = 0, 3
        if hasattr(args, 'n_levels'):
            args.n_levels = 5
        if hasattr(args, 'f_inner_stride'):
            args.f_inner_stride = 1
        assert call(ctypes.byref(args), None) == 0, lib.remap_last_error()
