#!/usr/bin/env python
"""Probe build of the library: compiles sar-ssl_amd/csrc with extra defines into tmp_ab/lib<name>.so and prints its path - load it
through SARSSL_HIP_LIB.  The shipped library reads no environment variable; the tuning probes that are still useful live behind
-DSARSSL_PROBE_ENV (SARSSL_FFN_ROT, SARSSL_SPLIT_FM, SARSSL_GEMM_FM, SARSSL_GRID_* / *_STREAMS), timing-only ablations of the fused
feed-forward kernels behind -DFFN_ABL=<mask> (wrong results by construction).

    export SARSSL_HIP_LIB=$(python tools/probe_lib.py envprobe -DSARSSL_PROBE_ENV)

An existing build of that name is reused; PROBE_REBUILD=1 compiles it again."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sar-ssl_amd", "csrc"))
import build as B  # noqa: E402


def probe_lib(name, defines):
    d = os.path.join(ROOT, "tmp_ab")
    os.makedirs(d, exist_ok=True)
    out = os.path.join(d, "lib%s.so" % name)
    if os.path.exists(out) and not os.environ.get("PROBE_REBUILD"):
        return out
    objs = [os.path.join(d, "%s_%s" % (name, s.replace(".hip", ".o"))) for s in B.SOURCES]
    with ThreadPoolExecutor(max_workers=4) as ex:
        list(ex.map(lambda so: subprocess.check_call([B._hipcc()] + B.FLAGS + list(defines) + ["-c", os.path.join(B.HERE, so[0]), "-o", so[1]]),
                    zip(B.SOURCES, objs)))
    subprocess.check_call([B._hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out] + objs + ["-lpthread", "-ldl"])
    return out


if __name__ == "__main__":
    print(probe_lib(sys.argv[1], sys.argv[2:]))
