"""CPU: what online simulated pretraining (--simu-online) adds on the host - the closed-form Sabine solve, the device-resident source
bank's plans against SourceBank.draw, the loader's items as pure functions of their global index, the command line, the ABI."""
import os
import re

import numpy as np
import pytest

import online_cases as oc
from conftest import ROOT

NS = 4352
T_SMALL = 0.272
SMALL = dict(room_sz_range=[(3, 4), (3, 4), (2.5, 3)], T60_range=(0.2, 0.4))


# ---------------------------------------------------------------------------------------------------------------- closed-form solve
def _t60error(x, T60, room_sz, w):
    alpha = x * w
    Sa = (alpha[0] + alpha[1]) * room_sz[1] * room_sz[2] + (alpha[2] + alpha[3]) * room_sz[0] * room_sz[2] + \
        (alpha[4] + alpha[5]) * room_sz[0] * room_sz[1]
    return T60 if Sa == 0 else abs(T60 - 0.161 * np.prod(room_sz) / Sa)


def test_closed_form_sabine_solve_is_never_worse_than_the_minimiser():
    from scipy.optimize import minimize
    from sar_ssl_amd import roomsim
    D = roomsim.DEFAULTS
    worst_beta = 0.0
    for seed in range(500):
        rs = np.random.RandomState(seed)
        room_sz = [rs.uniform(*r) for r in D["room_sz_range"]]
        T60 = rs.uniform(*D["T60_range"])
        abs_weights = [rs.uniform(*r) for r in D["abs_weights_range"]]
        x, w = roomsim.sabine_x_closed(room_sz, T60, abs_weights)
        assert 0.0 <= x <= 1.0 and np.array_equal(w, np.asarray(abs_weights) / np.max(abs_weights))
        xm = minimize(lambda v, *a: _t60error(v[0], *a), 0.5, args=(T60, room_sz, w), bounds=[[0, 1]]).x[0]
        assert _t60error(x, T60, room_sz, w) <= _t60error(xm, T60, room_sz, w) + 1e-12, seed
        beta = roomsim._beta_sabine_closed(room_sz, T60, abs_weights)
        assert beta.dtype == np.float32 and np.array_equal(beta, np.sqrt(1 - x * w).astype(np.float32))
        worst_beta = max(worst_beta, float(np.abs(beta - roomsim._beta_sabine_estimation(room_sz, T60, abs_weights)).max()))
    print("max |beta_closed - beta_minimiser| over 500 draws: %.2e" % worst_beta)


def test_random_room_keeps_the_minimiser_by_default():
    from sar_ssl_amd import roomsim
    for seed in range(12):
        a = roomsim.random_room(np.random.RandomState(seed))
        rs_b = np.random.RandomState(seed)
        b = roomsim.random_room(rs_b, beta_solver="minimize")
        rs_a = np.random.RandomState(seed)
        roomsim.random_room(rs_a)
        assert a["room_sz"] == b["room_sz"] and a["T60_specify"] == b["T60_specify"] and a["T60_sabine"] == b["T60_sabine"]
        assert a["beta"].tobytes() == b["beta"].tobytes()
        assert all(np.array_equal(x, y) for x, y in zip(rs_a.get_state()[1:3], rs_b.get_state()[1:3]))
        c = roomsim.random_room(np.random.RandomState(seed), beta_solver="closed")
        assert c["room_sz"] == a["room_sz"] and c["beta"].dtype == np.float32 and abs(c["T60_sabine"] - c["T60_specify"]) < 0.005
    cfg_a = roomsim.random_spatial_acoustics(np.random.RandomState(), 1, 5)
    cfg_b = roomsim.random_spatial_acoustics(np.random.RandomState(), 1, 5, beta_solver="minimize")
    assert all(np.array_equal(np.asarray(cfg_a[k]), np.asarray(cfg_b[k])) for k in cfg_a)
    with pytest.raises(ValueError, match="beta_solver"):
        roomsim.random_room(np.random.RandomState(0), beta_solver="newton")


# ---------------------------------------------------------------------------------------------------------------- source plan
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return oc.write_tree(tmp_path_factory.mktemp("spk"), single=100)


def test_device_source_bank_plans_what_source_bank_draws(tree):
    from sar_ssl_amd import rirsynth
    top, utts = tree
    host = rirsynth.SourceBank(top, oc.FS, sort=True)
    bank = rirsynth.DeviceSourceBank(top, oc.FS, "cpu", sort=True)
    assert len(bank) == len(host) == 3 and bank.flat.dtype.is_floating_point is False and bank.flat.dim() == 1
    assert bank.flat.numel() == sum(u.shape[0] for u in utts.values()) and bank.spk_ids == host.spk_ids
    nseg_seen = set()
    for nsample in (64, 250, NS):
        for seed in range(40):
            idx = seed % 3
            if host.spk_ids[idx] == "spkB" and nsample == NS:
                continue                                        # 44 repetitions of 100 samples: refused, below
            ra, rb = np.random.RandomState(seed), np.random.RandomState(seed)
            src, want = host.draw(ra, idx, nsample)
            got = bank.plan(rb, idx, nsample)
            assert {k: got[k] for k in want} == want
            assert all(np.array_equal(x, y) for x, y in zip(ra.get_state()[1:3], rb.get_state()[1:3]))
            flat = bank.flat.numpy()
            crop = oc.host_crop([flat[o:o + n] for o, n in got["segments"]], got["seg_start"], nsample)
            assert crop.tobytes() == src.astype(np.float32).tobytes(), (nsample, seed)
            assert bank.host_crop(got, nsample).tobytes() == src.tobytes()
            assert 1 <= len(got["segments"]) <= rirsynth.MAXSEG and 0 <= got["seg_start"] < got["segments"][0][1]
            nseg_seen.add((host.spk_ids[idx], len(got["segments"])))
    assert ("spkC", 1) in nseg_seen and ("spkB", 3) in nseg_seen and any(s == "spkA" and n >= 3 for s, n in nseg_seen)
    off, ln, nseg, start = bank.tables([got])
    assert off.shape == ln.shape == (1, 32) and off.dtype == np.int64 and ln.dtype == np.int32 and nseg.dtype == np.int32 and start.dtype == np.int64
    assert int(nseg[0]) == len(got["segments"]) and int(start[0]) == got["seg_start"]


def test_device_source_bank_refusals(tree, tmp_path):
    from sar_ssl_amd import rirsynth
    from sar_ssl_amd.dataset import write_wav_pcm16
    top, utts = tree
    bank = rirsynth.DeviceSourceBank(top, oc.FS, "cpu", sort=True)
    with pytest.raises(ValueError, match="44 utterances, more than MAXSEG = 32"):
        bank.plan(np.random.RandomState(0), bank.spk_ids.index("spkB"), NS)
    nbytes = 2 * sum(u.shape[0] for u in utts.values())
    with pytest.raises(ValueError, match="holds %d bytes of PCM-16.*max_bytes = %d: nothing is truncated" % (nbytes, nbytes - 2)):
        rirsynth.DeviceSourceBank(top, oc.FS, "cpu", max_bytes=nbytes - 2)
    assert rirsynth.DeviceSourceBank(top, oc.FS, "cpu", max_bytes=nbytes).flat.numel() * 2 == nbytes
    with pytest.raises(ValueError, match="sampling rate 16000, expected 8000"):
        rirsynth.DeviceSourceBank(top, 8000, "cpu")
    d = tmp_path / "tr" / "s" / "spk"
    d.mkdir(parents=True)
    write_wav_pcm16(str(d / "u.wav"), np.zeros((50, 2), np.int16), oc.FS)
    with pytest.raises(ValueError, match="2 channels"):
        rirsynth.DeviceSourceBank(str(tmp_path / "tr"), oc.FS, "cpu")


# ---------------------------------------------------------------------------------------------------------------- online plans
@pytest.fixture(scope="module")
def bank(tmp_path_factory):
    from sar_ssl_amd import rirsynth
    top, _ = oc.write_tree(tmp_path_factory.mktemp("spk2k"), single=2000)
    return rirsynth.DeviceSourceBank(top, oc.FS, "cpu", sort=True)


def _loader(bank, B=4, dataset_sz=12, **kw):
    from sar_ssl_amd import onlinesig
    return onlinesig.OnlineSignalLoader(bank, dataset_sz, B, T_SMALL, 1, "cpu", **dict(SMALL, **kw))


def _same(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    return True


def _epoch(ld, epoch):
    return [g for s in range(len(ld)) for g in ld.indices(epoch, s)]


def test_an_online_item_is_a_function_of_its_global_index(bank):
    a, b = _loader(bank, 4, chunk=8), _loader(bank, 6, chunk=1024)
    c = _loader(bank, 4, rank=1, world=3, noise="numpy")
    assert _epoch(a, 0) == _epoch(b, 0) == list(range(12)) and [len(a), len(b)] == [3, 2] and b.indices(0, 1) == list(range(6, 12))
    for g in (0, 5, 11, 12, 40):
        assert _same(a.item_cfg(g), b.item_cfg(g)) and _same(a.item_cfg(g), c.item_cfg(g))
        pa, pb, pc = a.item_plan(g), b.item_plan(g), c.item_plan(g)
        assert pa["white"] is None and pc["white"].shape == (NS, 2) and pc["white"].dtype == np.float64
        for p in (pb, dict(pc, white=None)):
            assert p == pa
        assert pa["idx"] == g and 15 <= pa["snr"] < 30 and 0 <= pa["src_idx"] < 3
        r = a.restate_plan(g)
        assert r["src"].shape == (NS,) and r["src"].dtype == np.float64 and abs(r["src"].mean()) < 1e-12 and _same(r["cfg"], a.item_cfg(g))
    assert not np.array_equal(a.item_cfg(0)["room_sz"], a.item_cfg(1)["room_sz"]) and a.item_plan(0) != dict(a.item_plan(1), idx=0)
    assert 3 <= a.item_cfg(0)["room_sz"][0] <= 4 and abs(a.item_cfg(0)["T60_sabine"] - a.item_cfg(0)["T60_specify"]) < 0.005
    other = _loader(bank, 4, dataset_sz=12)
    other.seed = 2
    assert not np.array_equal(other.item_cfg(0)["room_sz"], a.item_cfg(0)["room_sz"])


def test_online_ranks_and_epochs_partition_the_indices(bank):
    r0, r1 = _loader(bank, 4, dataset_sz=16, rank=0, world=2), _loader(bank, 4, dataset_sz=16, rank=1, world=2)
    e0 = [_epoch(r, 0) for r in (r0, r1)]
    assert len(r0) == len(r1) == 2 and not set(e0[0]) & set(e0[1]) and sorted(e0[0] + e0[1]) == list(range(16))
    assert e0[0] == [0, 1, 2, 3, 8, 9, 10, 11] and e0[1] == [4, 5, 6, 7, 12, 13, 14, 15]
    e1 = _epoch(r0, 1) + _epoch(r1, 1)
    assert sorted(e1) == list(range(16, 32)) and not set(e1) & set(e0[0] + e0[1])
    one = _loader(bank, 4, dataset_sz=10)
    assert len(one) == 3 and _epoch(one, 0) == list(range(10)) and one.indices(2, 2) == [28, 29]
    one.set_epoch(3)
    assert one.epoch == 3


def test_online_reuse_shares_the_room_and_not_the_signal(bank):
    ld = _loader(bank, 4, reuse=2)
    for k in range(4):
        assert _same(ld.item_cfg(2 * k), ld.item_cfg(2 * k + 1))
        pa, pb = ld.item_plan(2 * k), ld.item_plan(2 * k + 1)
        assert (pa["snr"], pa["crop_start"]) != (pb["snr"], pb["crop_start"])
    assert not np.array_equal(ld.item_cfg(1)["room_sz"], ld.item_cfg(2)["room_sz"])
    assert _same(ld.item_cfg(2), _loader(bank, 4).item_cfg(1))            # room 1 either way
    with pytest.raises(ValueError, match="reuse = 3 does not divide the batch size 4"):
        _loader(bank, 4, reuse=3)
    with pytest.raises(RuntimeError, match="GPU only"):
        next(iter(ld))


# ---------------------------------------------------------------------------------------------------------------- the command
def test_online_flags_parse():
    from sar_ssl_amd.opt import opt_pretrain
    o = opt_pretrain()
    a = o.parse(["--pretrain", "--simu-exp", "--gpu-id", "0,", "--work-dir", "/tmp/w"])
    assert a.simu_online is False and a.simu_online_reuse == 1 and a.simu_online_bank_gb == 8
    a = o.parse(["--pretrain", "--simu-exp", "--simu-online", "--simu-online-reuse", "4", "--simu-online-bank-gb", "2.5", "--gpu-id", "0,",
                 "--work-dir", "/tmp/w"])
    assert a.simu_online is True and a.simu_online_reuse == 4 and a.simu_online_bank_gb == 2.5
    assert o.dir()["srcsig_train"] == "/tmp/w/data/SrcSig/wsj0/tr"


@pytest.mark.parametrize("argv, what", [
    (["--test", "--simu-exp", "--simu-online"], "this command has --test"),
    (["--pretrain-frozen-encoder", "--simu-exp", "--simu-online"], "this command has --pretrain-frozen-encoder"),
    (["--pretrain", "--simu-online"], "this command has no --simu-exp"),
    (["--pretrain", "--simu-online-reuse", "2"], "this command has no --simu-exp"),
    (["--pretrain", "--simu-exp", "--simu-online-reuse", "2"], "give --simu-online with them"),
    (["--pretrain", "--simu-exp", "--simu-online", "--simu-online-reuse", "3", "--bs", "4", "4", "4"], "does not divide the training batch size 4"),
])
def test_invalid_online_commands_end_before_the_gpu_is_touched(monkeypatch, argv, what):
    import torch
    import sar_ssl_amd.run_pretrain as rp
    from sar_ssl_amd import launch
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(launch, "spawn_ranks", lambda *a, **k: pytest.fail("a rank was spawned"))
    for name in ("is_available", "set_device", "init", "device_count", "current_device"):
        monkeypatch.setattr(torch.cuda, name, lambda *a, **k: pytest.fail("torch.cuda was touched"))
    with pytest.raises(SystemExit) as e:
        rp.main(argv + ["--gpu-id", "0,", "--work-dir", "/tmp/w", "--time", "t0"])
    assert what in str(e.value) and "--simu-online" in str(e.value)


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_src_gather_is_declared_as_it_is_called():
    import ast
    from sar_ssl_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sarssl_hip.h")).read()
    m = re.search(r"int sarssl_src_gather\(([^)]*)\);", hdr)
    assert m is not None
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["const short* bank", "long bank_len", "const long* seg_off", "const int* seg_len", "const int* nseg",
                      "const long* crop_start", "int nb", "long ns", "void* ws", "long ws_bytes", "float* out", "void* stream"]
    kinds = ["ptr" if "*" in p else p.split()[0] for p in params]
    tree = ast.parse(open(os.path.join(ROOT, "sar-ssl_amd", "hip.py")).read())
    calls = [n for n in ast.walk(tree) if isinstance(n, ast.Call) and n.args and isinstance(n.args[0], ast.Constant)
             and n.args[0].value == "sarssl_src_gather"]
    assert len(calls) == 1
    wrap = {"_p": "ptr", "c_void_p": "ptr", "_stream": "ptr", "c_int": "int", "c_long": "long"}
    assert [wrap[a.func.id] for a in calls[0].args[1:]] == kinds
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    assert hasattr(_lib.lib(), "sarssl_src_gather") and _lib.lib().sarssl_abi_version() == 3
