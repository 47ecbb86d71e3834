"""GPU: the signal generator (gen_simu.py --mode sig, roomsim.simulate_signals) and its new kernels - sarssl_rir_labels against
roomsim.labels on identical f32 input (parity.RIRLABELS), sarssl_pcm16_pack against numpy bit for bit, the written files against the f64
restatement roomsim.restate_sig (parity.SIMSIG), the retry path, simulate_bank(labels="device") against labels="host", and the written
directory as input of the pretraining step."""
import json
import os

import numpy as np
import pytest
import torch

import recipes
import simsig_cases as sc
from conftest import GOLD, check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T_SMALL = 0.272
NS_SMALL = 4352


def _tol():
    from sar_ssl_amd import parity
    return {k: min(parity.RIRLABELS["gate"][k], parity.RIRLABELS["cap"][k]) for k in parity.RIRLABELS["gate"]}


_device_labels = sc.device_labels


# ---------------------------------------------------------------------------------------------------------------- the labels kernel
@pytest.mark.parametrize("nch", [1, 2, 3])
def test_rir_labels_against_the_host_labels(nch):
    tol, worst = _tol(), {}
    for case in sc.label_cases(nch):
        want = sc.host_labels(case[1], case[2], case[3])
        got = _device_labels([case])[0]
        try:
            dist = sc.same_labels(got, want, tol)
        except AssertionError as e:
            raise AssertionError("%s (nch %d): %s" % (case[0], nch, e))
        for k, v in dist.items():
            worst[k] = max(worst.get(k, 0.0), v)
    for k in ("t60", "corr", "drr", "c50"):
        check("rirlabels.nch%d.%s" % (nch, k), worst[k], tol[k])


def test_rir_labels_do_not_depend_on_batch_position_or_row_length():
    cases = {c[0]: c for c in sc.label_cases(2)}
    pick = [cases[n] for n in ("full_0.2_2049", "full_0.87_13867", "short_257", "all_zero", "plateau")]
    a = _device_labels(pick)
    order = [3, 0, 4, 2, 1]
    b = _device_labels([pick[i] for i in order], lmax=14001, ldmax=1700)
    tol = _tol()
    for j, i in enumerate(order):
        for k in a[i]:
            assert np.array_equal(a[i][k], b[j][k], equal_nan=True), (pick[i][0], k, a[i][k], b[j][k])
        sc.same_labels(a[i], sc.host_labels(pick[i][1], pick[i][2], pick[i][3]), tol)


def test_rir_labels_refuses_unsupported_bounds():
    from sar_ssl_amd import _lib, hip
    dev = torch.device(DEV)
    assert hip.rir_labels_workspace_bytes(2, 9, 100, 100) == -1 and hip.rir_labels_workspace_bytes(2, 2, 32769, 100) == -1
    assert hip.rir_labels_workspace_bytes(2, 2, 100, 0) == -1 and hip.rir_labels_workspace_bytes(2, 2, 32768, 32768) > 0
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)             # noqa: E731
    n = torch.ones(1, dtype=torch.int32, device=dev)
    with pytest.raises(_lib.SarsslHipError):
        hip.rir_labels(z(1, 9, 64), n, z(1, 9, 64), n, torch.zeros(1, dtype=torch.float64, device=dev))


# ---------------------------------------------------------------------------------------------------------------- float -> PCM-16
def test_pcm16_pack_is_bit_equal_to_numpy():
    from sar_ssl_amd import hip
    dev = torch.device(DEV)
    rs = np.random.RandomState(0)
    x = (rs.standard_normal((3, NS_SMALL, 2)) * 0.4).astype(np.float32)
    x[0, :8, 0] = [0.9, -0.9, 1.0, -1.0, 1.5, -1.5, 0.0, -0.0]
    # half-integer products.  32767 is odd, so x 32767 = m + 1/2 has the single solution |x| = 1/2 inside [-1, 1] (16383.5 -> 16384, the
    # even neighbour); (k + 1/2) / 32767 rounded to f32 is no longer a tie - its exact f64 product lies 1e-8 beside one, on the side an
    # f32 product would not see - and is kept as the near-tie case
    near = ((np.arange(-300, 300) + 0.5) / 32767.0).astype(np.float32)
    frac = np.abs(np.modf(near.astype(np.float64) * 32767.0)[0])
    assert (frac != 0.5).all() and (np.abs(frac - 0.5) < 1e-3).all()
    x[1, :near.size, 1] = near
    x[2, :4, 0] = [0.5, -0.5, 0.50001525, -0.50001525]
    assert np.rint(np.float64(x[2, 0, 0]) * 32767.0) == 16384 and np.float64(x[2, 0, 0]) * 32767.0 == 16383.5
    for ns in (1, 63, 64, 65, NS_SMALL):
        xs = np.ascontiguousarray(x[:, :ns])
        got = hip.pcm16_pack(torch.from_numpy(xs).to(dev)).cpu().numpy()
        want = np.clip(np.rint(xs.astype(np.float64) * 32767.0), -32767, 32767).astype(np.int16)
        assert got.dtype == np.int16 and got.shape == want.shape and np.array_equal(got, want), ns
    from sar_ssl_amd import roomsim
    assert np.array_equal(roomsim.pcm16(x), hip.pcm16_pack(torch.from_numpy(x).to(dev)).cpu().numpy())


# ---------------------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return sc.write_speech_tree(tmp_path_factory.mktemp("speech"), np.load(sc.F22))


def _simulate(tmp, tree, data_num, batch, noise="numpy", T=T_SMALL, stage="pretrain"):
    from sar_ssl_amd import roomsim
    lines = []
    res = roomsim.simulate_signals(str(tmp), stage, data_num, tree, device=DEV, noise=noise, batch=batch, T=T, sort_sources=True,
                                   log=lines.append, **sc.SMALL)
    return res, lines


def _plans(tree, ids, seed=1, T=T_SMALL):
    from sar_ssl_amd import rirsynth, roomsim
    rs = np.random.RandomState()
    draw = {k: v for k, v in dict(roomsim.DEFAULTS, **sc.SMALL).items() if k != "fs"}
    cfgs = {i: roomsim.random_spatial_acoustics(rs, seed, i, **draw) for i in ids}
    sources = rirsynth.SourceBank(os.path.join(tree, "tr"), sc.FS, sort=True)
    return {i: roomsim.plan_sig(rs, i, seed, cfgs[i], sources, T) for i in ids}


def _restated(plan, attempt=0, seed=1):
    from sar_ssl_amd import roomsim
    n_len = roomsim.plan_rir(plan["cfg"])["n_len"]
    return roomsim.restate_sig(plan, roomsim.numpy_noise(seed, plan["idx"], attempt, 2, n_len))


def _against_restatement(name, wav, want):
    """The pass conditions of a written file -> the share of samples that differ."""
    from sar_ssl_amd import parity
    from sar_ssl_amd.dataset import read_wav_pcm16
    pcm, fs = read_wav_pcm16(wav)
    assert fs == sc.FS and pcm.shape == want.shape and pcm.dtype == np.int16
    d = np.abs(pcm.astype(np.int32) - want.astype(np.int32))
    share = float((d != 0).mean())
    print("PARITY %s.max_step measured=%d tol=%d (at most)" % (name, d.max(), parity.SIMSIG["pcm_step"]))
    assert d.max() <= parity.SIMSIG["pcm_step"], (name, int(d.max()))
    check(name + ".share", share, parity.SIMSIG["share_bound"])
    assert np.abs(pcm).max() >= 29000                           # the peak of mic / direct path sits at 0.9 of full scale
    return share


@pytest.fixture(scope="module")
def e2e(tmp_path_factory, tree):
    tmp = tmp_path_factory.mktemp("sig8")
    res, lines = _simulate(tmp, tree, 8, 8)
    return tmp / "pretrain", res, lines, _plans(tree, range(8))


def test_small_rooms_end_to_end_against_the_restatement(e2e):
    out, res, lines, plans = e2e
    assert res["written"] == list(range(8)) and res["skipped"] == [] and lines == []
    assert all(res["attempts"][i] == 1 for i in range(8))
    shares = [_against_restatement("simsig.idx%d" % i, str(out / ("%d.wav" % i)), _restated(plans[i])) for i in range(8)]
    print("largest share of differing samples: %.4f" % max(shares))
    names = sorted(os.listdir(out))
    assert names == sorted(["%d.wav" % i for i in range(8)] + ["%d_info.npz" % i for i in range(8)] + ["all_info.npz"])
    all_info = np.load(out / "all_info.npz", allow_pickle=True)
    assert len(all_info["cfgs"]) == 8 and all_info["skipped"].size == 0 and all_info["args"].item()["stage"] == "pretrain"


def test_small_rooms_info_files(e2e):
    """{idx}_info.npz: the labels against roomsim.labels of the same RIRs (rendered again here, as the generator renders them, and read
    back), the draws exactly."""
    from sar_ssl_amd import roomsim
    out, res, lines, plans = e2e
    dev = torch.device(DEV)
    ids = list(range(8))
    lmax = roomsim.sig_lmax(sc.SMALL["T60_range"])
    batch = roomsim.render_items({i: plans[i]["cfg"] for i in ids}, ids, 1, 0, dev, noise="numpy", lmax=lmax)
    rp, dpp, rir, dp = batch.plans, batch.plans_dp, batch.rir.cpu().numpy(), batch.dp.cpu().numpy()
    assert max(p["n_len"] for p in rp) <= 4094 < lmax
    tol = _tol()
    for i in ids:
        info = dict(np.load(out / ("%d_info.npz" % i), allow_pickle=True))
        cfg = plans[i]["cfg"]
        want = roomsim.labels(rir[i, :, :rp[i]["n_len"]], dp[i, :, :dpp[i]["n_len"]], cfg)
        assert want["ok"] and abs(want["T60_edc"] - cfg["T60_specify"]) < 0.05 - 0.005
        check("simsig.info%d.T60_edc" % i, abs(float(info["T60_edc"]) - want["T60_edc"]), tol["t60"])
        for k in ("DRR", "C50"):
            assert info[k].dtype == np.float16
            # (rounded to float16 on both sides: equal, or neighbours where the unrounded values straddle a rounding boundary)
            assert info[k] == want[k] or abs(float(info[k]) - float(want[k])) <= float(np.spacing(np.float16(want[k]))), (k, info[k], want[k])
        assert info["TDOA"].dtype == np.float32 and info["TDOA"] == want["TDOA"]
        assert float(info["SNR"]) == plans[i]["snr"] and int(info["src_idx"]) == plans[i]["src_idx"]
        for k in cfg:
            assert np.array_equal(np.asarray(info[k]), np.asarray(cfg[k])), k
        assert sorted(info) == sorted(list(cfg) + ["T60_edc", "SNR", "src_idx", "TDOA", "DRR", "C50"])


def test_files_do_not_depend_on_the_batch(tmp_path, tree):
    a, _ = _simulate(tmp_path / "a", tree, 3, 3)
    b, _ = _simulate(tmp_path / "b", tree, 3, 1)
    assert a["written"] == b["written"] == [0, 1, 2]
    for i in range(3):
        for name in ("%d.wav" % i, "%d_info.npz" % i):
            fa, fb = tmp_path / "a" / "pretrain" / name, tmp_path / "b" / "pretrain" / name
            if name.endswith(".wav"):
                assert fa.read_bytes() == fb.read_bytes(), name
            else:
                ia, ib = np.load(fa, allow_pickle=True), np.load(fb, allow_pickle=True)
                assert sorted(ia.files) == sorted(ib.files) and all(np.array_equal(ia[k], ib[k]) for k in ia.files), name


def test_device_noise(tmp_path, tree, e2e):
    from sar_ssl_amd import roomsim
    from sar_ssl_amd.dataset import read_wav_pcm16
    res, lines = _simulate(tmp_path, tree, 4, 4, noise="device")
    assert res["written"] == [0, 1, 2, 3] and res["skipped"] == [] and max(res["attempts"].values()) <= roomsim.MAX_ATTEMPTS
    for i in range(4):
        pcm, fs = read_wav_pcm16(str(tmp_path / "pretrain" / ("%d.wav" % i)))
        other, _ = read_wav_pcm16(str(e2e[0] / ("%d.wav" % i)))
        assert pcm.shape == (NS_SMALL, 2) and fs == sc.FS and 29000 <= np.abs(pcm).max() <= 32767
        assert not np.array_equal(pcm, other)


def test_a_rejected_item_is_rendered_again_and_written_once(tmp_path, tree, monkeypatch):
    from sar_ssl_amd import roomsim
    judge, calls = roomsim.judge_on_device, []

    def failing_once(rir, n_len, rir_dp, dp_len, T60_specify, ids=None, attempt=0, fs=sc.FS):
        lab = judge(rir, n_len, rir_dp, dp_len, T60_specify, ids, attempt, fs)
        calls.append((list(ids), attempt))
        if attempt == 0:
            lab["flags"][list(ids).index(1)] = 1                # item 1: rir_ok without env_ok
        return lab

    monkeypatch.setattr(roomsim, "judge_on_device", failing_once)
    res, lines = _simulate(tmp_path, tree, 3, 3)
    assert calls == [([0, 1, 2], 0), ([1], 1)]
    assert res["written"] == [0, 1, 2] and res["skipped"] == [] and res["attempts"] == {0: 1, 1: 2, 2: 1}
    plans = _plans(tree, [1])
    _against_restatement("simsig.retry", str(tmp_path / "pretrain" / "1.wav"), _restated(plans[1], attempt=1))
    first = _restated(plans[1], attempt=0)
    from sar_ssl_amd.dataset import read_wav_pcm16
    assert (np.abs(read_wav_pcm16(str(tmp_path / "pretrain" / "1.wav"))[0].astype(np.int32) - first) > 1).any()
    assert sorted(os.listdir(tmp_path / "pretrain")) == sorted(["%d.wav" % i for i in range(3)] + ["%d_info.npz" % i for i in range(3)]
                                                               + ["all_info.npz"])


def test_an_item_that_never_passes_is_skipped_and_listed(tmp_path, tree, monkeypatch):
    from sar_ssl_amd import roomsim
    judge = roomsim.judge_on_device

    def never(rir, n_len, rir_dp, dp_len, T60_specify, ids=None, attempt=0, fs=sc.FS):
        lab = judge(rir, n_len, rir_dp, dp_len, T60_specify, ids, attempt, fs)
        if 0 in ids:
            lab["flags"][list(ids).index(0)] = 1
        return lab

    monkeypatch.setattr(roomsim, "judge_on_device", never)
    monkeypatch.setattr(roomsim, "MAX_ATTEMPTS", 2)
    res, lines = _simulate(tmp_path, tree, 2, 2)
    assert res["written"] == [1] and res["skipped"] == [0] and res["attempts"][0] == 2 and len(lines) == 1 and "item 0" in lines[0]
    assert not (tmp_path / "pretrain" / "0.wav").exists() and list(np.load(tmp_path / "pretrain" / "all_info.npz", allow_pickle=True)["skipped"]) == [0]


# ---------------------------------------------------------------------------------------------------------------- --mode rir
def test_simulate_bank_with_device_labels_writes_the_same_bank(tmp_path):
    from sar_ssl_amd import roomsim
    res = {}
    for where in ("host", "device"):
        res[where] = roomsim.simulate_bank(str(tmp_path / where), "train", 4, device=DEV, noise="numpy", batch=3, labels=where, log=print,
                                           **sc.SMALL)
    assert res["host"] == res["device"] and res["host"]["written"] == [0, 1, 2, 3]
    tol = _tol()
    for i in range(4):
        for name in ("%d.npy" % i, "%d_dp.npy" % i):
            assert (tmp_path / "host" / "train" / name).read_bytes() == (tmp_path / "device" / "train" / name).read_bytes(), name
        h = np.load(tmp_path / "host" / "train" / ("%d_info.npz" % i), allow_pickle=True)
        d = np.load(tmp_path / "device" / "train" / ("%d_info.npz" % i), allow_pickle=True)
        assert sorted(h.files) == sorted(d.files)
        for k in h.files:
            if k == "T60_edc":
                check("simbank.device_labels.T60_edc.%d" % i, abs(float(h[k]) - float(d[k])), tol["t60"])
                assert d[k].dtype == h[k].dtype
            else:
                assert h[k].dtype == d[k].dtype and np.array_equal(h[k], d[k]), (i, k, h[k], d[k])


@pytest.mark.parametrize("where", ["host", "device"])
def test_simulate_bank_renders_a_rejected_item_again(tmp_path, monkeypatch, where):
    """The retry path of --mode rir: item 1, rejected once (rir_ok without env_ok), is rendered again with attempt 1's noise and written
    once; the others, and every direct path, are attempt 0's.  Each file against a render of that item alone."""
    from sar_ssl_amd import roomsim
    seed, dev = roomsim.STAGE_SEEDS["train"], torch.device(DEV)
    judge, calls = getattr(roomsim, "judge_on_" + where), []

    def reject(lab, ids, attempt):
        calls.append((list(ids), attempt))
        if attempt == 0:
            lab["flags"][list(ids).index(1)] = 1
        return lab

    def on_host(batch, cfgs, fs=sc.FS, c=343.0):
        return reject(judge(batch, cfgs, fs, c), batch.ids, len(calls))        # (one batch per attempt here: the call count is the attempt)

    def on_device(rir, n_len, rir_dp, dp_len, T60_specify, ids=None, attempt=0, fs=sc.FS):
        return reject(judge(rir, n_len, rir_dp, dp_len, T60_specify, ids, attempt, fs), ids, attempt)

    monkeypatch.setattr(roomsim, "judge_on_" + where, on_host if where == "host" else on_device)
    res = roomsim.simulate_bank(str(tmp_path), "train", 3, device=DEV, noise="numpy", batch=3, labels=where, **sc.SMALL)
    assert calls == [([0, 1, 2], 0), ([1], 1)]
    assert res["written"] == [0, 1, 2] and res["skipped"] == [] and res["attempts"] == {0: 1, 1: 2, 2: 1}
    out = tmp_path / "train"
    assert sorted(os.listdir(out)) == sorted(["%d%s" % (i, s) for i in range(3) for s in (".npy", "_dp.npy", "_info.npz")] + ["all_info.npz"])
    cfgs = np.load(out / "all_info.npz", allow_pickle=True)["cfgs"]

    def alone(i, attempt=None):
        """Item i rendered by itself, read back in the files' layout: the RIR with ``attempt``'s uploaded noise, or the direct path."""
        plan = [roomsim.plan_rir(cfgs[i], dp=attempt is None)]
        noise = None if attempt is None else roomsim.host_noise(plan, [i], seed, attempt, dev)
        return roomsim.render(plan, dev, noise).cpu().numpy()[:, :, :, None]

    def same(name, want):
        got = np.load(out / name)
        return got.dtype == want.dtype == np.float32 and got.shape == want.shape and got.tobytes() == want.tobytes()

    assert same("1.npy", alone(1, 1)) and not same("1.npy", alone(1, 0))
    assert same("0.npy", alone(0, 0)) and same("2.npy", alone(2, 0))
    assert all(same("%d_dp.npy" % i, alone(i)) for i in range(3))


# ---------------------------------------------------------------------------------------------------------------- the product
def test_written_segments_feed_the_pretraining_step(tmp_path, tree):
    from sar_ssl_amd import dataset, hip, model, runtime
    res, lines = _simulate(tmp_path, tree, 4, 4, noise="device", T=4.112)
    assert res["written"] == [0, 1, 2, 3]
    files = sorted(str(p) for p in (tmp_path / "pretrain").glob("*.wav"))
    dev = torch.device(DEV)
    (pcm,) = next(iter(dataset.PcmSegmentLoader(files, batch_size=4, device=dev)))
    assert pcm.shape == (4, 65792, 2) and pcm.dtype == torch.int16 and int(pcm.abs().max()) >= 29000
    runtime.set_precision("hybrid")
    try:
        man = json.load(open(os.path.join(GOLD, "state_dict_manifest.json")))["pretrain"]
        net = model.SARSSL(sig_shape=(256, 256, 2, 2), pretrain=True, device=dev)
        net.load_state_dict(recipes.recipe_state_dict(man, 0))
        net.to(dev).train()
        flat = runtime.FlatParams(net)
        opt = runtime.FusedAdam(flat, lr=1e-4)
        opt.zero_grad()
        loss, _, _ = net(hip.stft_frontend(pcm))
        loss.backward()
        opt.step()
        assert bool(torch.isfinite(loss.detach())) and float(loss.detach()) > 0
    finally:
        runtime.set_precision("bf16")
