"""
Builds ``libremap_hip.so`` (the C-ABI HIP library, ``include/remap_hip.h``)
in-tree with hipcc for gfx950.  Used by ``__graft_entry__.build()`` and, as a
convenience, on first use when the library is missing but hipcc is present.
``build()`` also makes ``libremap_hip_wideindex.so`` beside it, for the tests
(``build_wide_index_library``).
"""
import os
import shutil
import subprocess

_PKG = os.path.dirname(os.path.abspath(__file__))
_REPO = os.path.dirname(_PKG)
CSRC = os.path.join(_PKG, 'csrc')
INCLUDE = os.path.join(_REPO, 'include')
LIB_DIR = os.path.join(_PKG, '_lib')
LIB_PATH = os.environ.get('REMAP_HIP_LIB') or \
    os.path.join(LIB_DIR, 'libremap_hip.so')
SOURCES = ['remap_spmm.hip', 'remap_csr.hip', 'remap_schedule.hip',
           'remap_plan.hip', 'remap_shard.hip', 'remap_overlap.hip',
           'remap_nearest.hip', 'remap_locate.hip', 'remap_quads.hip',
           'remap_expand.hip', 'remap_geometry.hip',
           'remap_conserve2nd.hip', 'remap_patch.hip', 'remap_limit.hip',
           'remap_sgs.hip', 'remap_vector.hip', 'remap_levels.hip',
           'remap_layers.hip']
ARCH = 'gfx950'
#: the row passes (rowpass.h) and the tests' build of them that takes the
#: 64-bit index instantiations on problems of any size: a test artefact the
#: package itself never loads (build_wide_index_library)
ROWPASS_SOURCES = ['remap_limit.hip', 'remap_sgs.hip', 'remap_vector.hip',
                   'remap_levels.hip', 'remap_layers.hip']
WIDE_LIB_PATH = os.path.join(LIB_DIR, 'libremap_hip_wideindex.so')
WIDE_DEFINE = '-DREMAP_ROWPASS_WIDE_INDEX'


def find_hipcc():
    for cand in (os.environ.get('HIPCC'), shutil.which('hipcc'),
                 '/opt/rocm/bin/hipcc'):
        if cand and os.path.exists(cand):
            return cand
    return None


def sources():
    return [os.path.join(CSRC, s) for s in SOURCES]


def _deps():
    return sources() + [os.path.join(INCLUDE, 'remap_hip.h'),
                        os.path.join(CSRC, 'libremap_hip.map')] + \
        [os.path.join(CSRC, f) for f in os.listdir(CSRC)
         if f.endswith('.h')]


def is_stale(lib_path=None):
    lib_path = lib_path or LIB_PATH
    if not os.path.exists(lib_path):
        return True
    built = os.path.getmtime(lib_path)
    return any(os.path.getmtime(d) > built for d in _deps())


def _compile(hipcc, names, obj_dir, defines, force, verbose):
    """One hipcc per source of ``names`` whose object in ``obj_dir`` is older
    than the source or a header, side by side; returns every object."""
    os.makedirs(obj_dir, exist_ok=True)
    # -fvisibility=hidden: the library's dynamic symbols are the REMAP_API
    # entry points of include/remap_hip.h and nothing else (no mangled
    # remap::... helpers, no kernel stubs)
    common = [hipcc, '-O3', '-std=c++17', f'--offload-arch={ARCH}',
              '-ffp-contract=off', '-fPIC', '-fvisibility=hidden',
              f'-I{INCLUDE}', f'-I{CSRC}'] + list(defines)
    headers = [os.path.join(INCLUDE, 'remap_hip.h')] + \
        [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith('.h')]
    newest_header = max(os.path.getmtime(h) for h in headers)
    jobs = []
    objs = []
    for name in names:
        src = os.path.join(CSRC, name)
        obj = os.path.join(obj_dir, name + '.o')
        objs.append(obj)
        fresh = os.path.exists(obj) and not force and \
            os.path.getmtime(obj) > max(os.path.getmtime(src), newest_header)
        if fresh:
            continue
        cmd = common + ['-c', src, '-o', obj]
        if verbose:
            print(' '.join(cmd))
        jobs.append((src, subprocess.Popen(
            cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
            text=True)))
    failed = []
    for src, proc in jobs:
        out, _ = proc.communicate()
        if proc.returncode != 0:
            failed.append(f'{src}:\n{out}')
    if failed:
        raise RuntimeError('hipcc failed:\n' + '\n'.join(failed))
    return objs


def _link(hipcc, objs, lib_path, verbose):
    cmd = [hipcc, f'--offload-arch={ARCH}', '-fPIC', '-shared',
           '-Wl,--version-script=' + os.path.join(CSRC, 'libremap_hip.map'),
           '-o', lib_path] + objs
    if verbose:
        print(' '.join(cmd))
    proc = subprocess.run(cmd, stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, text=True)
    if proc.returncode != 0:
        raise RuntimeError(f'hipcc (link) failed:\n{proc.stdout}')
    return lib_path


def build_library(force=False, verbose=False):
    """
    ``hipcc -O3 --offload-arch=gfx950 -ffp-contract=off -shared``.

    ``-ffp-contract=off`` keeps the multiply and the add of the accumulation
    separate, which is what makes the default mode bit-identical to scipy's
    ``csr_matvecs`` (the REMAP_FLAG_FMA kernels call fma explicitly).
    """
    if not force and not is_stale():
        return LIB_PATH
    hipcc = find_hipcc()
    if hipcc is None:
        raise RuntimeError('hipcc not found: cannot build libremap_hip.so')
    os.makedirs(LIB_DIR, exist_ok=True)
    # one hipcc per source, side by side (remap_spmm.hip alone takes over a
    # minute: hundreds of kernel instantiations), then one link
    objs = _compile(hipcc, SOURCES, os.path.join(LIB_DIR, 'obj'), [], force,
                    verbose)
    return _link(hipcc, objs, LIB_PATH, verbose)


def build_wide_index_library(force=False, verbose=False):
    """
    ``libremap_hip_wideindex.so``: the product's objects (``_lib/obj``, built
    first where they are missing or stale) with the five row passes compiled
    again under ``-DREMAP_ROWPASS_WIDE_INDEX`` into ``_lib/obj_wide``, the
    same flags otherwise and the same version script.  Its row passes take
    the 64-bit index instantiations on problems of any size, which the
    product takes from 2^32 elements a launch on; results are the product's.
    For tests/test_gpu_wide_index.py; nothing in the package loads it.
    """
    product = os.path.join(LIB_DIR, 'libremap_hip.so')
    if not force and not is_stale(WIDE_LIB_PATH) and \
            not is_stale(product) and \
            os.path.getmtime(WIDE_LIB_PATH) >= os.path.getmtime(product):
        return WIDE_LIB_PATH
    hipcc = find_hipcc()
    if hipcc is None:
        raise RuntimeError(
            'hipcc not found: cannot build libremap_hip_wideindex.so')
    os.makedirs(LIB_DIR, exist_ok=True)
    # (fresh objects are kept: this compiles what the product build left
    # stale, never remap_spmm.hip a second time)
    objs = _compile(hipcc, SOURCES, os.path.join(LIB_DIR, 'obj'), [], False,
                    verbose)
    wide = _compile(hipcc, ROWPASS_SOURCES, os.path.join(LIB_DIR, 'obj_wide'),
                    [WIDE_DEFINE], force, verbose)
    swapped = dict(zip(ROWPASS_SOURCES, wide))
    objs = [swapped.get(name, obj) for name, obj in zip(SOURCES, objs)]
    return _link(hipcc, objs, WIDE_LIB_PATH, verbose)
