"""he_vecnorm_attach_step without a GPU: the built code object's step1_vnw_kernel instances
(tools/kernel_meta.py, as test_kernel_meta_cpu.py), the ctypes declaration against the header's,
and the env limit's two copies."""
import ctypes
import importlib.util
import os
import re
import shutil
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "cantorrl_amd", "lib", "libhedgeenv.so")
HEADER = os.path.join(ROOT, "include", "hedge_env.h")


def test_step_kernels_hold_no_scratch_and_no_spilled_vgprs():
    """Replay, GBM (greeks from the tile or made in the kernel) and Heston, with the info fields
    (4 instances) and without (7: generate modes also FAST, as he_step's own kernels).  No scratch
    memory and no VGPR spills; the SGPR spills the metadata also counts go to VGPR lanes, not to
    memory (every he_step kernel with a fused epilogue reports them): the VGPR count, which
    includes those lanes, is what is bounded."""
    if not os.path.exists(LIB):
        pytest.skip("libhedgeenv.so not built")
    for tool in ("llvm-readelf", "clang-offload-bundler"):
        if not os.path.exists(os.path.join("/opt/rocm/lib/llvm/bin", tool)):
            pytest.skip(f"{tool} absent")
    if shutil.which("objcopy") is None:
        pytest.skip("objcopy absent")
    spec = importlib.util.spec_from_file_location("kernel_meta", os.path.join(ROOT, "tools", "kernel_meta.py"))
    km = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(km)
    meta = {}
    with tempfile.TemporaryDirectory() as td:
        for co in km.code_objects(LIB, td):
            meta.update(km.metadata(co))
    vnw = {k: v for k, v in meta.items() if "step1_vnw_kernel" in k}
    assert len(vnw) == 11, sorted(vnw)
    plain = {v["lds_B"] for k, v in meta.items() if "step1_kernel" in k}

    def targs(sym, name):   # the template arguments of a mangled kernel name, as ints
        m = re.search(name + r"I((?:L[ib]\d+E)+)E", sym)
        return tuple(int(x) for x in re.findall(r"L[ib](\d+)E", m.group(1)))
    # step_kernel<MODE, INFO, SINGLE, BOOK, FAST, POL, GS>: an armed instance exists for a (mode,
    # info, greeks) combination exactly where he_step has a kernel of its own
    step = {targs(k, "step_kernel") for k in meta if "11step_kernelI" in k}
    for k, v in sorted(vnw.items()):
        print(k, v)
        assert v["scratch_B"] == 0 and v["vgpr_spill"] == 0, (k, v)
        # SGPR spills live in lanes of VGPRs that the VGPR count includes (64 per VGPR): with no
        # scratch they never reach memory, and the count stays within the library's 128-VGPR
        # budget (4 waves per SIMD) with them.  he_step's kernels with an epilogue fused in
        # (step1_vn_kernel, step1_vne_kernel) hold theirs the same way.
        assert v["vgpr"] <= 128, (k, v)
        mode, info, book, fast, gs = targs(k, "step1_vnw_kernel")
        assert not (info and fast) and not book and (mode, info, 1, 0, 0, 0, gs) in step, (k, v)
        # two obs tiles and the statistics' and sums' buffers, in a launch of one workgroup: the
        # library's bound for a kernel that leaves room for four workgroups on a CU
        assert v["lds_B"] <= 40 * 1024, (k, v)
    assert plain == {13312}, plain   # the plain step kernels are other instances: their one obs tile, as before


def _header():
    with open(HEADER) as f:
        return f.read()


def test_ctypes_declaration_matches_the_header():
    from cantorrl_amd import _lib
    m = re.search(r"^he_status\s+he_vecnorm_attach_step\(([^)]*)\);", _header(), re.M)
    assert m, "he_vecnorm_attach_step is not declared in include/hedge_env.h"
    params = [re.sub(r"\s+\w+$", "", p.strip()) for p in m.group(1).split(",")]   # drop the names
    ctype = {"he_env*": ctypes.c_void_p, "void*": ctypes.c_void_p,
             "const he_vecnorm_params*": ctypes.POINTER(_lib.HeVecnormParams),
             "const he_vecnorm_out*": ctypes.POINTER(_lib.HeVecnormOut)}
    res, args = _lib.SIG["he_vecnorm_attach_step"]
    assert res is ctypes.c_int32   # he_status
    assert args == [ctype[p] for p in params], (params, args)
    assert "he_vecnorm_attach_step" in _lib.EXPORTS


def test_env_limit_matches_the_header():
    from cantorrl_amd import _lib
    m = re.search(r"^#define\s+HE_VN_STEP_MAX_ENVS\s+(\d+)\s*$", _header(), re.M)
    assert m and int(m.group(1)) == _lib.HE_VN_STEP_MAX_ENVS == 256
