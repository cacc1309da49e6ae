"""The Python mirrors of the public structs against the headers themselves: a small C program that
includes the header prints sizeof and every field's offsetof as the host C compiler lays them out,
and the ctypes structures / numpy record dtypes must say the same.  A field added to a header and
not to its mirror changes sizeof or an offset; one the header does not have does not compile.  Either
fails here instead of corrupting a call."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")


def _mirrors(header):
    """[(C struct name, its Python mirror)] of one header."""
    if header == "hedge_env.h":
        from cantorrl_amd import _lib
        return [("he_book_option", _lib.HeBookOption), ("he_config", _lib.HeConfig), ("he_info", _lib.HeInfo),
                ("he_vecnorm_params", _lib.HeVecnormParams), ("he_vecnorm_out", _lib.HeVecnormOut),
                ("he_episode_record", _lib.EPISODE_RECORD)]
    if header == "rbergomi.h":
        from cantorrl_amd import rbergomi
        return [("rb_base_params", rbergomi.RbBaseParams), ("rb_config", rbergomi.RbConfig)]
    from cantorrl_amd import agent
    pytest.importorskip("torch")   # cantorrl_amd.train imports it
    from cantorrl_amd import train
    return [("ha_weights", agent.HaWeights), ("ha_policy_weights", agent.HaPolicyWeights),
            ("ha_episode_sums", agent.EPISODE_SUMS), ("ha_lstm_seq_net", train.HaLstmSeqNet),
            ("ha_lstm_seq_bwd", train.HaLstmSeqBwd), ("ha_lstm_seq_wgrad", train.HaLstmSeqWgrad),
            ("ha_adam_tensor", train.HaAdamTensor), ("ha_adam_hyper", train.HaAdamHyper)]


def _python_layout(mirror):
    """(size, {field: offset}) of a ctypes.Structure or a numpy record dtype."""
    if isinstance(mirror, np.dtype):
        return mirror.itemsize, {f: mirror.fields[f][1] for f in mirror.names}
    return ctypes.sizeof(mirror), {f[0]: getattr(mirror, f[0]).offset for f in mirror._fields_}


@pytest.mark.parametrize("header", ["hedge_env.h", "rbergomi.h", "hedge_actor.h"])
def test_python_mirrors_match_the_header(header, tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler (cc, gcc, clang) on the path")
    mirrors = _mirrors(header)
    lines = []
    for cname, mirror in mirrors:
        lines.append(f'    printf("{cname} %zu\\n", sizeof({cname}));')
        for f in _python_layout(mirror)[1]:
            lines.append(f'    printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    src = tmp_path / "abi.c"
    src.write_text(f'#include <stddef.h>\n#include <stdio.h>\n#include "{header}"\n'
                   "int main(void) {\n" + "\n".join(lines) + "\n    return 0;\n}\n")
    exe = tmp_path / "abi"
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    c_side = {k: int(v) for k, v in (ln.split() for ln in out.splitlines())}
    py_side = {}
    for cname, mirror in mirrors:
        size, offsets = _python_layout(mirror)
        py_side[cname] = size
        py_side.update({f"{cname}.{f}": o for f, o in offsets.items()})
    assert py_side == c_side
    # the sizes as they were measured when this test was written (a check of the test itself)
    known = {"he_config": 528, "he_info": 216, "he_vecnorm_params": 64, "he_vecnorm_out": 72, "he_episode_record": 80}
    assert all(c_side[k] == v for k, v in known.items() if k in c_side)

