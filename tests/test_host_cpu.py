"""CPU tests of the host side: C-ABI exports, state_dict layout, mask RNG order, schedule, WAV I/O, flat-parameter
bookkeeping, and that the product path refuses to run without a GPU (no CPU fallback)."""
import json
import os
import random
import re

import numpy as np
import pytest
import torch

import recipes
from conftest import GOLD, ROOT


def test_cabi_library_exports_every_declared_symbol():
    import __graft_entry__ as g
    from sar_ssl_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    lib = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "sarssl_hip.h")).read()
    names = sorted(set(re.findall(r"\b(sarssl_[a-z0-9_]+)\s*\(", hdr)))
    assert len(names) >= 35
    for n in names:
        assert hasattr(lib, n), "missing export: " + n
    assert lib.sarssl_abi_version() == 3
    # collectives: RCCL is resolved with dlopen at first use - the answer needs no GPU, and the library loaded without librccl linked in
    assert lib.sarssl_comm_available() in (0, 1)
    if lib.sarssl_comm_available():
        assert lib.sarssl_comm_rccl_version() > 20000


def test_cabi_library_exports_nothing_but_the_declared_symbols():
    """The other direction of the test above: every dynamic symbol of the library that starts with sarssl_ is declared in the header (the
    three stamp buffers of a probe build excepted), so a retired entry point cannot stay behind as an export."""
    import shutil
    import subprocess
    from sar_ssl_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libsarssl_hip.so is not built")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    nm = shutil.which("nm") or shutil.which("llvm-nm") or shutil.which("llvm-nm", path=os.path.join(rocm, "llvm", "bin"))
    assert nm is not None, "neither nm nor ROCm's llvm-nm found"
    out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("sarssl_")}
    declared = set(_header_prototypes())
    probe = {"sarssl_conv_stamp_buffer", "sarssl_gemm_stamp_buffer", "sarssl_ffn_stamp_buffer"}
    assert len(declared) >= 148 and exported - probe == declared, (sorted(exported - probe - declared), sorted(declared - exported))


_C_SCALARS = ("int", "long", "float", "double", "unsigned long long", "unsigned int")


def _c_kind(text, named, stmt):
    """'ptr' or the scalar's C type of one parameter (``named``: drop the parameter's name) or of the return type."""
    if "*" in text:
        return "ptr"
    words = [w for w in text.split() if w != "const"]
    k = " ".join(words[:-1] if named else words)
    assert k in _C_SCALARS, "unknown type `%s` in: %s" % (text, stmt)
    return k


def _header_prototypes(text=None):
    """{entry point: (return kind, [parameter kinds])} read from include/sarssl_hip.h (or ``text``)."""
    hdr = open(os.path.join(ROOT, "include", "sarssl_hip.h")).read() if text is None else text
    src = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    src = re.sub(r"^\s*#.*$", " ", src, flags=re.M).replace('extern "C" {', " ")
    protos = {}
    for stmt in src.split(";"):
        stmt = " ".join(stmt.split()).strip("} ")
        if "sarssl_" not in stmt or stmt.startswith("typedef "):
            continue
        m = re.match(r"^([\w\s*]+?)\s*\b(sarssl_\w+)\s*\(([^()]*)\)$", stmt)
        assert m is not None, "unreadable declaration: " + stmt
        params = [a.strip() for a in m.group(3).split(",")] if m.group(3).strip() not in ("", "void") else []
        protos[m.group(2)] = (_c_kind(m.group(1), False, stmt), [_c_kind(a, True, stmt) for a in params])
    return protos


_WRAPPER_KIND = {"c_int": "int", "c_long": "long", "c_float": "float", "c_ulonglong": "unsigned long long", "c_double": "double",
                 "c_void_p": "ptr", "c_char_p": "ptr", "_p": "ptr", "_stream": "ptr", "byref": "ptr", "data_as": "ptr",
                 "create_string_buffer": "ptr"}


def _wrapper_kind(node):
    """Kind a call-site argument is wrapped as (None where the expression does not say: a name, an array constructor)."""
    import ast
    if isinstance(node, ast.IfExp):
        kinds = {_wrapper_kind(node.body), _wrapper_kind(node.orelse)} - {None}
        return kinds.pop() if len(kinds) == 1 else "mixed" if kinds else None
    if isinstance(node, ast.Call):
        fn = node.func.id if isinstance(node.func, ast.Name) else node.func.attr if isinstance(node.func, ast.Attribute) else None
        return _WRAPPER_KIND.get(fn)
    return None


def _abi_sites(source, path="<source>"):
    """Every way into the library in one Python file -> (sites, restypes).
    sites: (entry point, line, argument nodes, scope, direct, certain) of
      * ``<x>.call("sarssl_name", ...)`` with a literal name (direct False: _lib.call sets nothing on the function and checks the status),
      * ``<x>.sarssl_name(...)`` - the attribute-style call on the CDLL -, and
      * ``fn(...)`` where the enclosing function (or the module) holds ``fn = <x>.sarssl_name``;
      calls with a starred argument are left out; certain False: the receiver is not recognisably the library (an oracle function of
      the same prefix), the site counts only if the header knows the name.  restypes: (entry point, line, name of the assigned ctypes type, scope) of every
      ``<x>.sarssl_name.restype = T`` / ``fn.restype = T``.  scope: line of the enclosing def, 0 for the module."""
    import ast
    tree = ast.parse(source, path)
    sites, restypes, done = [], [], set()

    def entry(node, alias):
        if isinstance(node, ast.Attribute) and node.attr.startswith("sarssl_"):
            return node.attr
        return alias.get(node.id) if isinstance(node, ast.Name) else None

    def on_library(node):          # lib().x, _lib.lib().x, lib.x, L.x, _lib.x or a local alias: certainly the CDLL, so x must be declared
        r = node.value if isinstance(node, ast.Attribute) else None
        if isinstance(r, ast.Call):
            r = r.func
        return r is None or (r.attr if isinstance(r, ast.Attribute) else getattr(r, "id", None)) in ("lib", "_lib", "L")

    scopes = [tree] + [n for n in ast.walk(tree) if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef, ast.Lambda))]
    for scope in sorted(scopes, key=lambda n: -getattr(n, "lineno", 0)):            # innermost first: a site belongs to its nearest def
        sline = getattr(scope, "lineno", 0)
        nodes = sorted((n for n in ast.walk(scope) if hasattr(n, "lineno")), key=lambda n: (n.lineno, n.col_offset))
        alias = {}
        for n in nodes:
            if isinstance(n, ast.Assign) and len(n.targets) == 1 and isinstance(n.targets[0], ast.Name) and entry(n.value, {}):
                alias[n.targets[0].id] = n.value.attr
        for n in nodes:
            key = (type(n).__name__, n.lineno, n.col_offset)
            if key in done:
                continue
            if isinstance(n, ast.Assign):
                for t in n.targets:
                    targets = t.elts if isinstance(t, ast.Tuple) else [t]
                    values = n.value.elts if isinstance(t, ast.Tuple) and isinstance(n.value, ast.Tuple) else [n.value] * len(targets)
                    for tt, v in zip(targets, values):
                        if isinstance(tt, ast.Attribute) and tt.attr == "restype" and entry(tt.value, alias):
                            ty = v.attr if isinstance(v, ast.Attribute) else v.id if isinstance(v, ast.Name) else None
                            restypes.append((entry(tt.value, alias), n.lineno, ty, sline))
                            done.add(key)
            elif isinstance(n, ast.Call) and not any(isinstance(a, ast.Starred) for a in n.args):
                if (isinstance(n.func, ast.Attribute) and n.func.attr == "call" and n.args and isinstance(n.args[0], ast.Constant)
                        and isinstance(n.args[0].value, str) and n.args[0].value.startswith("sarssl_")):
                    sites.append((n.args[0].value, n.lineno, n.args[1:], sline, False, True))
                    done.add(key)
                elif entry(n.func, alias):
                    sites.append((entry(n.func, alias), n.lineno, n.args, sline, True, on_library(n.func)))
                    done.add(key)
    return sorted(sites, key=lambda s: s[1]), sorted(restypes, key=lambda r: r[1])


# sarssl_wall_clock_khz returns long, and bench.py / tools/step_stamps.py read it through the untyped default (int): the constant-rate
# device clock in kHz (1e5 on this part) is far below 2^31, so nothing is cut.  Every other long is a byte count and must be declared.
_LONG_THAT_FITS_INT = {"sarssl_wall_clock_khz"}
_RESTYPE_OF = {"long": "c_long", "ptr": ("c_void_p", "c_char_p")}


def _check_abi_file(path, source, protos, probe, at_load=()):
    """Asserts on one file; -> (sites, argument kinds compared, entry points seen).  at_load: names whose restype the loader (_lib.lib())
    sets on the CDLL every caller shares."""
    sites, restypes = _abi_sites(source, path)
    nkinds, seen = 0, set()
    for name, line, args, scope, direct, certain in sites:
        where = "%s:%d: %s" % (path, line, name)
        want = protos[name][1] if name in protos else probe.get(name)
        if want is None and not certain:
            continue
        assert want is not None, where + " is not declared in include/sarssl_hip.h"
        assert len(args) == len(want), "%s takes %d arguments, %d passed" % (where, len(want), len(args))
        for i, (arg, k) in enumerate(zip(args, want)):
            got = _wrapper_kind(arg)
            if got is not None:
                assert got == k, "%s: argument %d is wrapped as %s, the header says %s" % (where, i + 1, got, k)
                nkinds += 1
        ret = protos[name][0] if name in protos else "int"
        if direct and ret == "long" and name not in _LONG_THAT_FITS_INT:
            # a byte count read through the default restype (int) comes back cut to 32 bits: c_long, set in this function before the call
            assert any(r[0] == name and r[2] == "c_long" and r[3] == scope and r[1] <= line for r in restypes), \
                where + " returns long: set restype = c_long in front of the call"
        if direct and ret == "ptr":
            # handles and strings: declared when the library loads, or in this file
            assert name in at_load or any(r[0] == name and r[2] in _RESTYPE_OF["ptr"] for r in restypes), \
                where + " returns a pointer: restype is not set, here or at load"
        seen.add(name)
    for name, line, ty, _ in restypes:
        ret = protos[name][0] if name in protos else "int"
        assert ty == "c_int" if ret == "int" else ty in _RESTYPE_OF[ret], "%s:%d: %s.restype = %s, the header says %s" % (path, line, name, ty, ret)
    return sum(1 for s in sites if s[0] in seen), nkinds, seen


def _check_every_entry_point_is_called(protos, called):
    """Every entry point the header declares has a call site: an export nobody calls is a signature nothing checks and a body nothing
    runs (forwarding shims of older names piled up that way)."""
    idle = sorted(set(protos) - set(called))
    assert not idle, "declared in include/sarssl_hip.h without a call site: " + ", ".join(idle)


def test_cabi_call_sites_agree_with_the_header():
    """The call sites wrap every argument by hand (c_int / c_long / c_float / c_ulonglong / pointers) and ctypes checks none of it: a
    c_int where the header says long, a dropped or swapped argument, a byte count read without ``restype = c_long`` would show on the GPU
    only.  This walks both ways into the library - `call("sarssl_...", ...)` with a literal name, and the attribute-style calls on the
    CDLL (`lib().sarssl_x(...)`, also through a local `fn = lib().sarssl_x`) - in the package, the tools and the drivers, and compares
    argument count, wrapper kinds and the assigned return types with the header's prototypes (probe-build symbols, which the header does
    not declare, take one pointer).  The other way round, every declared entry point has a call site in those files or in the tests."""
    import glob
    protos = _header_prototypes()
    hdr = open(os.path.join(ROOT, "include", "sarssl_hip.h")).read()
    assert sorted(protos) == sorted(set(re.findall(r"\b(sarssl_[a-z0-9_]+)\s*\(", hdr))) and len(protos) >= 148
    assert {"sarssl_istft_workspace_bytes", "sarssl_wall_clock_khz", "sarssl_conv3x3_wgrad_workspace_bytes", "sarssl_dwglu_wgrad_workspace_bytes",
            "sarssl_layernorm_bwd_workspace_bytes", "sarssl_dwconv_wgrad_workspace_bytes",
            "sarssl_step_state_bytes"} <= {n for n, (r, _) in protos.items() if r == "long"}
    assert {"sarssl_comm_create", "sarssl_create", "sarssl_last_error"} <= {n for n, (r, _) in protos.items() if r == "ptr"}
    probe = {"sarssl_conv_stamp_buffer": ["ptr"], "sarssl_gemm_stamp_buffer": ["ptr"], "sarssl_ffn_stamp_buffer": ["ptr"]}
    files = [os.path.join(ROOT, "bench.py"), os.path.join(ROOT, "__graft_entry__.py")]
    for d in ("sar-ssl_amd", "tools"):
        files += glob.glob(os.path.join(ROOT, d, "**", "*.py"), recursive=True)
    loader = os.path.join(ROOT, "sar-ssl_amd", "_lib.py")
    at_load = {r[0] for r in _abi_sites(open(loader).read())[1]}
    assert {"sarssl_create", "sarssl_last_error"} <= at_load
    nsites, nkinds, seen, per_file = 0, 0, set(), {}
    for path in sorted(files):
        rel = os.path.relpath(path, ROOT)
        n, k, names = _check_abi_file(rel, open(path).read(), protos, probe, at_load)
        per_file[rel] = n
        nsites, nkinds, seen = nsites + n, nkinds + k, seen | names
    # the scan really finds the sites: 148 prototypes; 129 literal call(...) sites and 39 attribute-style ones today, 149 names called
    # (146 entry points and the three probe-build symbols), 1505 wrapped arguments
    assert nsites >= 162 and len(seen) >= 133 and nkinds >= 1427, (nsites, len(seen), nkinds)
    hip = os.path.join("sar-ssl_amd", "hip.py")
    direct = [s for s in _abi_sites(open(os.path.join(ROOT, hip)).read())[0] if s[4]]
    assert len(direct) >= 25 and {"sarssl_gemm_group_tn", "sarssl_layernorm_bwd_workspace_bytes", "sarssl_conv3x3_wgrad_workspace_bytes",
                                  "sarssl_colsum_slices", "sarssl_comm_create", "sarssl_step_state_skipped"} <= {s[0] for s in direct}
    assert per_file[os.path.join("sar-ssl_amd", "_lib.py")] >= 5 and per_file["__graft_entry__.py"] >= 1 and per_file["bench.py"] >= 1
    # the other direction: the tests count as callers (they read sarssl_ctx_device / sarssl_ctx_get_conv_cus), their arguments are not checked
    in_tests = set()
    for path in glob.glob(os.path.join(ROOT, "tests", "**", "*.py"), recursive=True):
        in_tests |= {s[0] for s in _abi_sites(open(path).read(), path)[0]}
    assert {"sarssl_ctx_device", "sarssl_ctx_get_conv_cus"} <= in_tests - seen
    _check_every_entry_point_is_called(protos, seen | in_tests)


def test_cabi_call_site_scan_catches_what_it_is_for(tmp_path):
    """The scan of test_cabi_call_sites_agree_with_the_header on small sources with one mistake each."""
    import ast
    protos = _header_prototypes()
    assert protos["sarssl_glu_fwd"] == ("int", ["ptr", "long", "int", "ptr", "int", "ptr"])
    assert protos["sarssl_layernorm_bwd_workspace_bytes"] == ("long", ["long", "int"])
    assert _wrapper_kind(ast.parse("_p(x) if x is not None else c_void_p(0)").body[0].value) == "ptr"
    assert _wrapper_kind(ast.parse("c_int(1) if x else c_long(0)").body[0].value) == "mixed"
    ok = ('def f(M, d):\n    fn = _lib.lib().sarssl_layernorm_bwd_workspace_bytes\n    fn.restype = c_long\n'
          '    n = fn(c_long(M), c_int(d))\n    _lib.call("sarssl_glu_fwd", _p(h), c_long(M), c_int(d), _p(g), c_int(1), _stream())\n'
          '    return bool(_lib.lib().sarssl_ffn2_supported(c_long(M), c_int(d)))\n')
    assert _check_abi_file("ok.py", ok, protos, {})[:2] == (3, 10)
    for old, new, what in (
            ("c_long(M), c_int(d), _p(g)", "c_int(M), c_int(d), _p(g)", "argument 2 is wrapped as int, the header says long"),
            ("c_int(d), _p(g), c_int(1)", "c_int(d), _p(g)", "takes 6 arguments, 5 passed"),
            ("fn(c_long(M), c_int(d))", "fn(c_int(M), c_int(d))", "argument 1 is wrapped as int, the header says long"),
            ("fn(c_long(M), c_int(d))", "fn(c_long(M))", "takes 2 arguments, 1 passed"),
            ("    fn.restype = c_long\n", "", "returns long: set restype = c_long"),
            ("fn.restype = c_long", "fn.restype = c_int", "returns long: set restype = c_long"),
            ("sarssl_ffn2_supported(c_long(M), c_int(d))", "sarssl_ffn2_supported(c_int(M), c_int(d))", "argument 1 is wrapped as int"),
            ("sarssl_ffn2_supported(", "sarssl_ffn3_supported(", "is not declared"),
            ("    return bool", "    c = L.sarssl_comm_create(c_int(n), c_int(r), buf)\n    return bool", "returns a pointer: restype is not set, here or at load")):
        assert old in ok
        with pytest.raises(AssertionError, match=re.escape(what)):
            _check_abi_file("bad.py", ok.replace(old, new), protos, {})
    # a restype set in another function does not count for a byte count
    with pytest.raises(AssertionError, match="returns long"):
        _check_abi_file("bad.py", ok.replace("    fn.restype = c_long\n", "") + "def g():\n    _lib.lib().sarssl_layernorm_bwd_workspace_bytes.restype = c_long\n",
                        protos, {})
    # a declared entry point nobody calls
    two = _header_prototypes("int sarssl_glu_fwd(const void* h, long M, int d, void* g, int dtype, void* stream);\nint sarssl_idle(int a);\n")
    called = _check_abi_file("ok.py", ok, protos, {})[2]
    _check_every_entry_point_is_called({"sarssl_glu_fwd": two["sarssl_glu_fwd"]}, called)
    with pytest.raises(AssertionError, match="without a call site: sarssl_idle\\n"):
        _check_every_entry_point_is_called(two, called)
    # the header reader names what it cannot read
    for text, what in (("int sarssl_x(int a, size_t n);", "unknown type `size_t n`"), ("void sarssl_x(int a);", "unknown type `void`"),
                       ("int sarssl_x(int (*cb)(int));", "unreadable declaration")):
        with pytest.raises(AssertionError, match=re.escape(what)):
            _header_prototypes("/* c */\n#ifndef H\nint sarssl_ok(const float* p, unsigned long long s);\n" + text + "\n#endif\n")


def test_state_dict_layout_matches_reference_manifest():
    from sar_ssl_amd import model
    man = json.load(open(os.path.join(GOLD, "state_dict_manifest.json")))
    net = model.SARSSL(sig_shape=(256, 256, 2, 2), pretrain=True, device="cpu")
    sd = net.state_dict()
    assert list(sd.keys()) == list(man["pretrain"].keys())
    assert all(list(v.shape) == man["pretrain"][k] for k, v in sd.items())
    assert sum(p.numel() for p in net.parameters()) == man["nparams_pretrain"] == 17534224
    ds = model.SARSSL(sig_shape=(256, 64, 2, 2), pretrain=False, device="cpu", downstream_embed="spat")
    assert list(ds.state_dict().keys()) == list(man["downstream"].keys())
    # sinusoid table identical to the reference's persistent buffer recipe
    import recipes
    assert torch.equal(sd["spec_encoder.embed.layers.0.sequential.1.module.positional_encoding.pe"], recipes.pe_table(512))


def test_no_cpu_fallback():
    from sar_ssl_amd import model, _lib
    net = model.SARSSL(sig_shape=(16, 8, 2, 2), patch_shape=(16, 1), pretrain=True, device="cpu")
    with pytest.raises(_lib.SarsslHipError):
        net(torch.randn(2, 2, 16, 8, 2))
    from sar_ssl_amd.common.Conformer import ConformerBlock
    with pytest.raises(_lib.SarsslHipError):
        ConformerBlock(encoder_dim=32, num_attention_heads=4)(torch.randn(2, 16, 32))
    from sar_ssl_amd import learner
    with pytest.raises(_lib.SarsslHipError):
        learner.STFTLearner(net, 512, 0.5, 512, 1, 16000).cpu()


def test_patch_mask_rng_order_matches_reference():
    from sar_ssl_amd.common.utils_module import PatchMask
    z = np.load(os.path.join(GOLD, "f4_masks.npz"))
    for seed in (0, 7, 123456):
        pm = PatchMask(patch_mode="T", nmasked_patch=128, npatch_shape=[1, 256], device="cpu")
        random.seed(seed)
        idx, ch = pm.sample(4, 2)
        assert np.array_equal(idx, z["seed%d.idx" % seed]) and np.array_equal(ch, z["seed%d.ch" % seed][:, 0])
        random.seed(seed)
        md, mpd, mcd, idx_t, ch_t = pm.forward((4, 256, 8, 2, 2))       # dense API form
        assert np.array_equal(idx_t.numpy(), idx) and md.shape == (4, 256, 8, 2)
        b = 1
        masked_frames = (mpd[b, :, 0, 0] == 0).nonzero().flatten().numpy()
        assert np.array_equal(np.sort(idx[b]), masked_frames)
        assert float(mcd[b, 0, 0, int(ch[b])]) == 0.0 and float(mcd[b, 0, 0, 1 - int(ch[b])]) == 1.0
        assert float(md.sum()) == 4 * 256 * 8 * 2 - 4 * 128 * 8


def test_lr_schedule_and_opt():
    from sar_ssl_amd.common.utils import create_learning_rate_schedule
    from sar_ssl_amd.opt import opt_pretrain
    z = np.load(os.path.join(GOLD, "f8_schedule.npz"))
    fn = create_learning_rate_schedule(total_steps=30, base=0.001, decay_type="cosine", warmup_steps=1, linear_end=1e-6)
    np.testing.assert_allclose([float(fn(e)) for e in range(1, 31)], z["lr"], rtol=1e-6)
    o = opt_pretrain()
    a = o.parse(["--pretrain", "--simu-exp", "--gpu-id", "0,", "--work-dir", "/tmp/w"])
    assert a.bs == [128, 128, 128] and a.lr == 0.001 and a.nepoch == 30 and a.seed == 1 and a.workers == 8
    assert o.dir()["micsig_simu_pretrain"] == "/tmp/w/SAR-SSL/data/MicSig/simu/pretrain"
    with pytest.raises(AssertionError):
        opt_pretrain().parse(["--pretrain", "--test"])


def test_wav_dataset_roundtrip(tmp_path):
    from sar_ssl_amd import dataset, synth
    segs = synth.make_batch(0, 3, nsample=4096)
    pcm = synth.to_pcm16(segs)
    for i in range(3):
        dataset.write_wav_pcm16(str(tmp_path / ("%d.wav" % i)), pcm[i])
    dataset.write_wav_pcm16(str(tmp_path / "0_dp.wav"), pcm[0])            # must be ignored
    ds = dataset.FixMicSigDataset(str(tmp_path), fs=16000, load_anno=False, dataset_sz=None)
    assert len(ds) == 3
    got = {tuple(ds[i][0].shape) for i in range(3)}
    assert got == {(4096, 2)} and ds[0][0].dtype == np.float32
    names = [os.path.basename(str(f)) for f in ds.files]
    k = names.index("1.wav")
    np.testing.assert_array_equal(ds[k][0], pcm[1].astype(np.float32) / 32768.0)
    raw = dataset.FixMicSigDataset(str(tmp_path), fs=16000, load_anno=False, dataset_sz=2, raw_pcm=True)
    assert len(raw) == 2 and raw[0][0].dtype == np.int16


def test_flat_params_bookkeeping_cpu():
    from sar_ssl_amd import runtime
    m = torch.nn.Sequential(torch.nn.Linear(5, 3), torch.nn.Linear(3, 2))
    ref = [p.detach().clone() for p in m.parameters()]
    flat = runtime.FlatParams(m)
    assert not flat.on_gpu and flat.numel % 8 == 0
    for p, r, o in zip(m.parameters(), ref, flat.offsets):
        assert torch.equal(p.data, r) and o % 8 == 0
        assert p.data.data_ptr() == flat.flat.data_ptr() + 4 * o and p.grad.data_ptr() == flat.grad.data_ptr() + 4 * o
    m(torch.randn(4, 5)).sum().backward()                      # autograd accumulates into the flat views
    assert float(flat.grad.abs().sum()) > 0
    flat.zero_grad()
    assert float(flat.grad.abs().sum()) == 0
    sl = flat.bucket_slices(2)
    assert sl[0][0] == 0 and sl[-1][1] == flat.numel and all(a[1] == b[0] for a, b in zip(sl[:-1], sl[1:]))


def test_synth_segments_are_deterministic():
    from sar_ssl_amd import synth
    a, b = synth.make_segment(5, nsample=2048), synth.make_segment(5, nsample=2048)
    assert np.array_equal(a, b) and a.shape == (2048, 2) and abs(np.abs(a).max() - 0.9) < 1e-6
    assert not np.array_equal(a, synth.make_segment(6, nsample=2048))


def test_native_wav_batch_reader_and_segment_loader(tmp_path):
    """the threaded PCM-16 reader of the C-ABI library against the pure-Python parser, its error reporting, and the
    prefetching segment loader's batching / sharding semantics (host-only code: runs without a GPU)."""
    from sar_ssl_amd import dataset, _lib
    rng = np.random.default_rng(0)
    n, ns, nch = 11, 3000, 2
    pcm = rng.integers(-32768, 32767, size=(n, ns, nch), dtype=np.int16)
    for i in range(n):
        dataset.write_wav_pcm16(str(tmp_path / ("%d.wav" % i)), pcm[i])
    dataset.write_wav_pcm16(str(tmp_path / "3_dp.wav"), pcm[3])                    # direct-path companions are not segments
    files = sorted(dataset.segment_files(str(tmp_path)), key=lambda p: int(p.stem))
    assert len(files) == n and dataset.wav_probe(files[0]) == (nch, 16000, ns)
    for nthreads in (1, 4):
        got = dataset.read_wav_batch(files, ns, nch, fs=16000, nthreads=nthreads)
        assert got.dtype == torch.int16 and np.array_equal(got.numpy(), pcm)
    part = dataset.read_wav_batch(files[:3], 1000, nch, offset=500)
    assert np.array_equal(part.numpy(), pcm[:3, 500:1500])
    ref0, fs0 = dataset.read_wav_pcm16(str(files[5]))
    assert fs0 == 16000 and np.array_equal(ref0, pcm[5])
    # WAVE_FORMAT_EXTENSIBLE header + an odd-sized LIST chunk before the data chunk
    import struct
    body = pcm[0].tobytes()
    fmt = struct.pack("<HHIIHHHHIH14s", 0xFFFE, nch, 16000, 16000 * nch * 2, nch * 2, 16, 22, 16, 3, 1, b"\x00" * 14)
    lst = b"LIST" + struct.pack("<I", 5) + b"abcde" + b"\x00"
    blob = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + lst + b"data" + struct.pack("<I", len(body)) + body
    with open(tmp_path / "ext.wav", "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(blob)) + blob)
    assert np.array_equal(dataset.read_wav_batch([tmp_path / "ext.wav"], ns, nch).numpy()[0], pcm[0])
    assert np.array_equal(dataset.read_wav_pcm16(str(tmp_path / "ext.wav"))[0], pcm[0])
    # loud failures: too short, wrong channel count, wrong rate, not a WAV, missing
    for bad, kw, msg in ((files[:2], dict(nsample=ns + 1), "need"), (files[:2], dict(nch=3), "channels"),
                         (files[:2], dict(fs=8000), "sample rate"), ([tmp_path / "nope.wav"], {}, "cannot open")):
        args = dict(nsample=ns, nch=nch, fs=16000)
        args.update(kw)
        with pytest.raises(_lib.SarsslHipError, match=msg):
            dataset.read_wav_batch(bad, args["nsample"], args["nch"], fs=args["fs"])
    (tmp_path / "junk.wav").write_bytes(b"not a wave file at all")
    with pytest.raises(_lib.SarsslHipError, match="RIFF"):
        dataset.read_wav_batch([tmp_path / "junk.wav"], 10, 2)
    # loader: sequential order, ragged last batch, drop_last, two-rank sharding with wrap-around padding, epoch reshuffle
    ld = dataset.PcmSegmentLoader(files, batch_size=4, fs=16000, nthreads=2)
    batches = [b[0].clone() for b in ld]
    assert len(ld) == 3 and [b.shape[0] for b in batches] == [4, 4, 3]
    assert np.array_equal(torch.cat(batches).numpy(), pcm)
    assert len(dataset.PcmSegmentLoader(files, batch_size=4, drop_last=True)) == 2
    seen = []
    for rank in range(2):
        ld = dataset.PcmSegmentLoader(files, batch_size=3, shuffle=True, seed=5, rank=rank, world=2, drop_last=True)
        ld.set_epoch(1)
        got = torch.cat([b[0].clone() for b in ld]).numpy()
        assert got.shape[0] == 6
        seen += [int(np.where((pcm == g).all(axis=(1, 2)))[0][0]) for g in got]
    assert len(set(seen)) >= 10                                                    # 12 draws from a wrapped permutation of 11
    ld1 = dataset.PcmSegmentLoader(files, batch_size=3, shuffle=True, seed=5, rank=0, world=2, drop_last=True)
    ld1.set_epoch(1)
    ld2 = dataset.PcmSegmentLoader(files, batch_size=3, shuffle=True, seed=5, rank=0, world=2, drop_last=True)
    ld2.set_epoch(2)
    assert ld1._order() != ld2._order() and sorted(ld1._order() + dataset.PcmSegmentLoader(
        files, batch_size=3, shuffle=True, seed=5, rank=1, world=2)._order_for(1)) == sorted(list(range(n)) + [ld1._order_all(1)[0]])
    # early break does not hang the producer thread
    it = iter(dataset.PcmSegmentLoader(files, batch_size=2, nthreads=2))
    next(it)
    it.close()


def test_native_mask_sampler_is_bit_identical_to_python_random():
    """The C-ABI mask sampler (sarssl_mask_sample) advances Python's own Mersenne Twister: same indices, same channels and the
    same generator state afterwards as random.sample / random.randint, for the shapes of configs 1-5."""
    import random
    from sar_ssl_amd.common import utils_module as um
    assert um._native_sampler_ok()
    for seed, (nb, n, k) in enumerate([(64, 256, 128), (8, 256, 128), (3, 624, 312), (5, 64, 32), (2, 16, 8), (1, 1045, 6)]):
        random.seed(1000 + seed)
        want = um._python_sample(nb, n, k, 2)
        state_want = random.getstate()
        random.seed(1000 + seed)
        got = um._native_sample(nb, n, k, 2)
        assert np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1]) and random.getstate() == state_want
        assert random.random() == (random.setstate(state_want) or random.random())     # the stream continues identically
    pm = um.PatchMask("T", 128, [1, 256], "cpu")
    z = np.load(os.path.join(GOLD, "f4_masks.npz"))
    random.seed(0)
    idx, ch = pm.sample(4, 2)
    key = [k for k in z.files if k.endswith(".idx")][0]
    seed0 = int(key.split(".")[0].replace("seed", ""))
    random.seed(seed0)
    idx, ch = pm.sample(4, 2)
    assert np.array_equal(idx, z["seed%d.idx" % seed0]) and np.array_equal(ch.reshape(-1), z["seed%d.ch" % seed0].reshape(-1))


def test_reference_written_checkpoint_file_matches_our_state_dict_layout():
    """Fixture F6 on the host: the file the reference's ``save_checkpoint`` wrote (fp32 layout: epoch / max_score / model) loads
    strictly into this build's MCConformer - same keys, shapes and values (code/learner.py:354-374)."""
    import gzip
    import io
    from sar_ssl_amd import model
    meta = np.load(os.path.join(GOLD, "f6_checkpoint_meta.npz"))
    with gzip.open(os.path.join(GOLD, "f6_checkpoint.tar.gz"), "rb") as f:
        ck = torch.load(io.BytesIO(f.read()), map_location="cpu", weights_only=False)
    assert set(ck.keys()) == {"epoch", "max_score", "model"} and ck["epoch"] == int(meta["epoch"])
    assert ck["max_score"] == float(meta["max_score"])
    net = model.MCConformer(sig_shape=[16, 8, 2, 2], patch_shape=(16, 1), dembed={"spec": 32, "spat": 32}, device="cpu")
    man = json.loads(str(meta["manifest_json"]))
    assert {k: list(v.shape) for k, v in net.state_dict().items()} == man
    net.load_state_dict(ck["model"], strict=True)
    want = recipes.recipe_state_dict(man, int(meta["weight_seed"]))
    for k, v in net.state_dict().items():
        assert torch.equal(v, want[k]), k


def test_dropout_replay_draws_the_reference_masks():
    """runtime.DropoutReplay: ``nn.Dropout`` on the CPU path is x * empty_like(x).bernoulli_(1 - p) / (1 - p) with consecutive
    draws from torch's global generator - what the replay reproduces (also for the conv module's (B, d, T) draw order)."""
    from sar_ssl_amd import runtime
    drop = torch.nn.Dropout(0.1).train()
    x1, x2 = torch.randn(3, 5, 8, requires_grad=True) + 4, torch.randn(2, 6, 7) + 4
    torch.manual_seed(123)
    y1, y2 = drop(x1), drop(x2)
    rp = runtime.DropoutReplay()
    torch.manual_seed(123)
    m1 = rp.mask((3, 5, 8), 0.1, "cpu", torch.float32)
    m2 = rp.mask((2, 6, 7), 0.1, "cpu", torch.float32, to_layout=lambda m: m.permute(0, 2, 1).reshape(14, 6))
    assert rp.draws == 2
    assert torch.allclose(y1.detach(), x1.detach() * m1) and torch.allclose(y2.permute(0, 2, 1).reshape(14, 6), x2.permute(0, 2, 1).reshape(14, 6) * m2)


def test_repeated_mask_indices_are_refused():
    """Advisor (round 5): the compact loss maps a masked frame to its row by counting the masked frames below it - a repeated index would
    silently shift rows.  PatchMask draws without replacement; forced masks with a repeat are refused on the host."""
    import numpy as np
    import pytest
    import torch
    from sar_ssl_amd import model
    net = model.SARSSL(sig_shape=(256, 8, 2, 2), pretrain=True, device="cpu")
    net.set_masks(np.array([[0, 2, 2, 5]]), np.array([0]))
    with pytest.raises(ValueError, match="distinct"):
        net._masks(1, 8, torch.device("cpu"))
    net.set_masks(np.array([[5, 0, 2, 7]]), np.array([1]))
    idx, ch, mp = net._masks(1, 8, torch.device("cpu"))
    assert idx.tolist() == [[0, 2, 5, 7]] and mp.tolist() == [[0, 1, 0, 1, 1, 0, 1, 0]]


def test_next_drop_reads_the_incoming_dropout_of_the_record_on_top():
    """engine._next_drop hands the LayerNorm backward the (p, seed, gscale) of the dropout backward that the next module of the backward
    chain applies to its incoming gradient: each module record's ``drop_in``, whatever else the record holds - and nothing where there is
    no mask to apply, the masks are replayed host tensors, or nobody / a consumer without dropout follows."""
    from sar_ssl_amd import engine

    def rec(kind, p, seed, g):
        if kind == "ffn":       # the output dropout (p2, s2) and the module factor - not the hidden layer's (p1, s1)
            return engine.FfnRec(x=None, ln=None, stats=None, hpre=None, a=None, p1=0.3, s1=11, p2=p, s2=seed, factor=g)
        if kind == "conv":
            return engine.ConvRec(x=None, ln=None, stats=None, h=None, g=None, c=None, aff=None, s=None, po=p, so=seed, B=2, T=16, train=True)
        return engine.MhsaRec(x=None, ln=None, stats=None, qu=None, qv=None, k=None, v=None, pos=None, pe=None, core=engine.ATTN_POS, bias=None,
                              ctx32=None, lse=None, p=None, pd=None, pa=0.2, sa=13, ctx=None, po=p, so=seed, B=2, T=16)

    for kind, g in (("ffn", 0.5), ("conv", 1.0), ("mhsa", 1.0)):
        below = rec("conv" if kind != "conv" else "ffn", 0.7, 99, 1.0)            # only the record on top counts
        got = engine._next_drop(kind, [below, rec(kind, 0.1, 1234, g)])
        assert got == (0.1, 1234, g) and [type(v) for v in got] == [float, int, float], kind
        assert engine._next_drop(kind, [rec(kind, 0.1, torch.ones(4), g)]) is None, kind          # a replayed mask
        assert engine._next_drop(kind, [rec(kind, 0.0, 0, 1.0)]) is None, kind                     # nothing to apply
        assert engine._next_drop(None, [rec(kind, 0.1, 1234, g)]) is None
        assert engine._next_drop("copy", [rec(kind, 0.1, 1234, g)]) is None
        assert engine._next_drop(kind, []) is None
    # the feed-forward module's factor alone is a reason to write the second output (p = 0, gscale = 0.5)
    assert engine._next_drop("ffn", [rec("ffn", 0.0, 0, 0.5)]) == (0.0, 0, 0.5)
    assert engine._next_drop("ffn", [rec("ffn", torch.tensor(0.1), 5, 0.5)]) is None
