"""GPU: the stored direct-path signal - sarssl_rir_mix_dp (hip.rir_mix(out_dp=...)) against rirsynth.restate_mix(return_dp=True) at the
gate of the mix itself, the stretch the kernel skips, the scale, ragged batches; roomsim.simulate_signals(save_dp=True) against
roomsim.restate_sig(with_dp=True) (parity.SIMSIG), its retry path; and the written corpus as input of run_pretrain.py --test --test-mode ins.

out_dp is filled with NaN before every kernel call: an element the kernels leave out fails the comparison."""
import os

import numpy as np
import pytest
import torch

import simsig_cases as sc
from conftest import check
from test_gpu_rirmix import N0, SNRS, _dev, _item

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T_SMALL = 0.272
NS_SMALL = 4352
STAGE = "pretest_ins_T1000"
SEED = 3000000                   # roomsim.SIG_STAGE_SEEDS['pretest'], which pretest_ins* takes


def _gate():
    from sar_ssl_amd import parity
    return min(parity.RIRMIX["gate"], parity.RIRMIX["cap"])


def _render(items, nch, explicit, with_noise=True, with_dp=True, lmax=None, ldmax=None):
    """items as in tests/test_gpu_rirmix.py -> (out, out_dp) (B, Ns, nch) numpy; out_dp None with with_dp=False.  Rows past an item's
    rir_len / dp_len hold 7.0, which must never be read; lmax / ldmax: the row lengths (default: the batch's longest)."""
    from sar_ssl_amd import hip
    B, Ns = len(items), items[0]["src"].shape[0]
    lmax = lmax or max(it["rir"].shape[1] for it in items)
    rir = np.full((B, nch, lmax), 7.0, np.float32)
    for b, it in enumerate(items):
        rir[b, :, :it["rir"].shape[1]] = it["rir"]
    if explicit:
        ldmax = ldmax or max(it["rir_dp"].shape[1] for it in items)
        dp = np.full((B, nch, ldmax), 7.0, np.float32)
        for b, it in enumerate(items):
            dp[b, :, :it["rir_dp"].shape[1]] = it["rir_dp"]
        kw = dict(rir_dp=_dev(dp), dp_len=_dev(np.array([it["rir_dp"].shape[1] for it in items]), torch.int32))
    else:
        kw = dict(n0=N0)
    noise = _dev(np.stack([it["noise"] for it in items])) if with_noise else None
    out_dp = torch.full((B, Ns, nch), float("nan"), dtype=torch.float32, device="cuda") if with_dp else None
    out = hip.rir_mix(_dev(np.stack([it["src"] for it in items])), _dev(rir),
                      _dev(np.array([it["rir"].shape[1] for it in items]), torch.int32),
                      _dev(np.array([it["snr"] for it in items])), _dev(np.array([it["gain"] for it in items])), noise=noise, out_dp=out_dp,
                      **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), (out_dp.cpu().numpy() if with_dp else None)


def _restate(it, explicit, with_noise=True):
    from sar_ssl_amd import rirsynth
    return rirsynth.restate_mix(it["src"], it["rir"], rir_dp=it["rir_dp"] if explicit else None, n0=None if explicit else N0,
                                noise=it["noise"] if with_noise else None, snr_db=it["snr"], gain=it["gain"], return_dp=True)


def _worst(out, out_dp, items, explicit, with_noise=True):
    """-> (largest distance of out, of out_dp) from the restatement; NaN (an unwritten element) counts as infinite."""
    w = [0.0, 0.0]
    for b, it in enumerate(items):
        for k, (got, want) in enumerate(zip((out[b], out_dp[b]), _restate(it, explicit, with_noise))):
            d = np.abs(got - want).max()
            w[k] = max(w[k], float("inf") if np.isnan(d) else float(d))
    return w


# ---------------------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("nch", [1, 2, 3])
@pytest.mark.parametrize("Ns", [256, 1000, 4352])
def test_rir_mix_dp_against_the_restatement(Ns, nch):
    """One ragged batch per (Ns, nch), as tests/test_gpu_rirmix.py renders it: explicit and windowed direct paths, with and without
    noise; out is bit-identical to the call without out_dp."""
    rs = np.random.RandomState(2000 * nch + Ns)
    Ls = [1, 255, 256, 257, 700, Ns + 300]
    items = [_item(rs, Ns, L, nch, snr=SNRS[i % 3], gain=(0.9, 1.0)[i % 2]) for i, L in enumerate(Ls)]
    worst = 0.0
    for explicit in (True, False):
        for with_noise in (True, False):
            out, out_dp = _render(items, nch, explicit, with_noise)
            plain, _ = _render(items, nch, explicit, with_noise, with_dp=False)
            assert np.isfinite(out_dp).all() and torch.equal(torch.from_numpy(out), torch.from_numpy(plain)), (explicit, with_noise)
            w_out, w_dp = _worst(out, out_dp, items, explicit, with_noise)
            assert w_out < _gate(), (explicit, with_noise, w_out)
            worst = max(worst, w_dp)
    check("rir_mix_dp Ns=%d nch=%d" % (Ns, nch), worst, _gate())


def test_rir_mix_dp_late_direct_path_is_exactly_zero_in_front():
    """Window mode, Ns = 4352 (17 blocks, three workgroups per filter), the RIR's signed maximum at sample 2300: the window 2260..2340
    lives in partitions 8 and 9, no live partition reaches output blocks 0..7, and the first workgroup of the direct path returns early -
    having written its 2048 zeros."""
    Ns, L, nch, peak = NS_SMALL, 2600, 2, 2300
    rs = np.random.RandomState(11)
    it = _item(rs, Ns, L, nch, snr=10.0)
    it["rir"] = (0.05 * rs.standard_normal((nch, L)) * np.exp(-np.arange(L) / 800.0)).astype(np.float32)
    it["rir"][:, peak] = 1.0
    assert list(np.argmax(it["rir"], axis=1)) == [peak] * nch and (peak - N0) // 256 == 8 and (peak + N0) // 256 == 9
    out, out_dp = _render([it], nch, False)
    plain, _ = _render([it], nch, False, with_dp=False)
    assert np.array_equal(out, plain)
    assert np.array_equal(out_dp[:, :2048], np.zeros((1, 2048, nch), np.float32))
    assert np.isfinite(out_dp).all() and np.abs(out_dp[:, 2048:]).max() > 0.01
    w_out, w_dp = _worst(out, out_dp, [it], False)
    assert w_out < _gate()
    check("rir_mix_dp late direct path", w_dp, _gate())
    # one channel only: the odd channel count's unpaired filter takes the same branch
    it1 = dict(it, rir=it["rir"][:1], noise=it["noise"][:, :1])
    out, out_dp = _render([it1], 1, False)
    assert np.array_equal(out_dp[:, :2048], np.zeros((1, 2048, 1), np.float32)) and np.isfinite(out_dp).all()
    check("rir_mix_dp late direct path, one channel", _worst(out, out_dp, [it1], False)[1], _gate())


def test_rir_mix_dp_peaks_at_the_gain_when_the_direct_path_sets_the_scale():
    """RIR = +1 at p and -0.9 at p + 1 against an explicit direct path +1 at p and a low-pass source: the reverberant signal nearly
    cancels (its peak is the source's onset), max|dp| is the divisor, and out_dp's peak is dp_peak / dp_peak * gain = gain exactly."""
    from sar_ssl_amd import hip, roomsim
    Ns, nch, p = 1000, 2, 37
    rs = np.random.RandomState(12)
    src = np.convolve(rs.standard_normal(Ns + 63), np.hanning(64) / np.hanning(64).sum(), mode="valid").astype(np.float32)
    rir = np.zeros((nch, p + 2), np.float32)
    rir[:, p], rir[:, p + 1] = 1.0, -0.9
    dp = np.zeros((nch, p + 1), np.float32)
    dp[:, p] = 1.0
    gain = np.float32(0.9)
    it = dict(src=src, rir=rir, rir_dp=dp, noise=np.zeros((Ns, nch), np.float32), snr=20.0, gain=float(gain))
    mic64, dp64 = _restate(it, True, with_noise=False)
    assert np.abs(dp64).max() > 1.2 * np.abs(mic64).max() and abs(np.abs(dp64).max() - float(gain)) < 1e-12
    out, out_dp = _render([it], nch, True, with_noise=False)
    assert np.abs(out_dp).max() == gain and np.abs(out).max() < gain / 1.2
    w_out, w_dp = _worst(out, out_dp, [it], True, with_noise=False)
    assert w_out < _gate()
    check("rir_mix_dp direct path sets the scale", w_dp, _gate())
    pcm = hip.pcm16_pack(torch.from_numpy(out_dp).cuda()).cpu().numpy()
    assert int(np.abs(pcm.astype(np.int32)).max()) == int(np.rint(0.9 * 32767)) == 29490
    assert np.array_equal(pcm, roomsim.pcm16(out_dp))


def test_rir_mix_dp_ragged_batch_equals_each_item_alone():
    rs = np.random.RandomState(13)
    items = [_item(rs, 1000, L, 2, snr=s, Ld=Ld) for L, Ld, s in ((300, 17, -5.0), (513, 300, 0.0), (900, 1, 30.0))]
    out, out_dp = _render(items, 2, True)
    w_out, w_dp = _worst(out, out_dp, items, True)
    assert w_out < _gate()
    check("rir_mix_dp ragged", w_dp, _gate())
    for b, it in enumerate(items):
        for rows in (dict(), dict(lmax=900, ldmax=300)):             # at its own row lengths, and at the batch's
            a, a_dp = _render([it], 2, True, **rows)
            assert np.array_equal(a[0], out[b]) and np.array_equal(a_dp[0], out_dp[b]), (b, rows)


def test_rir_mix_dp_refuses_a_missing_or_misshapen_out_dp():
    from sar_ssl_amd import _lib, hip
    rs = np.random.RandomState(14)
    it = _item(rs, 256, 64, 2)
    args = (_dev(it["src"][None]), _dev(it["rir"][None]), _dev(np.array([64]), torch.int32), _dev(np.array([0.0])), _dev(np.array([0.9])))
    with pytest.raises(AssertionError):
        hip.rir_mix(*args, n0=N0, out_dp=torch.empty((1, 256, 3), dtype=torch.float32, device="cuda"))
    lib = _lib.lib()
    assert hasattr(lib, "sarssl_rir_mix_dp") and lib.sarssl_abi_version() == 3
    ws = torch.empty(int(1 << 20), dtype=torch.uint8, device="cuda")
    out = torch.empty((1, 256, 2), dtype=torch.float32, device="cuda")
    p = hip._p
    with pytest.raises(_lib.SarsslHipError, match="out_dp"):
        _lib.call("sarssl_rir_mix_dp", p(args[0]), p(args[1]), p(args[2]), p(None), p(None), _lib.c_int(N0), p(None), p(args[3]), p(args[4]),
                  _lib.c_int(1), _lib.c_long(256), _lib.c_int(2), _lib.c_int(64), _lib.c_int(0), p(ws), p(out), p(None), hip._stream())


# ---------------------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return sc.write_speech_tree(tmp_path_factory.mktemp("speech_dp"), np.load(sc.F22))


def _simulate(tmp, tree, data_num, batch, save_dp=True, T=T_SMALL, noise="numpy"):
    from sar_ssl_amd import roomsim
    lines = []
    res = roomsim.simulate_signals(str(tmp), STAGE, data_num, tree, device=DEV, noise=noise, batch=batch, T=T, sort_sources=True,
                                   log=lines.append, save_dp=save_dp, **sc.SMALL)
    return res, lines


def _plans(tree, ids, T=T_SMALL):
    from sar_ssl_amd import rirsynth, roomsim
    rs = np.random.RandomState()
    draw = {k: v for k, v in dict(roomsim.DEFAULTS, **sc.SMALL).items() if k != "fs"}
    cfgs = {i: roomsim.random_spatial_acoustics(rs, SEED, i, **draw) for i in ids}
    sources = rirsynth.SourceBank(os.path.join(tree, "et"), sc.FS, sort=True)
    return {i: roomsim.plan_sig(rs, i, SEED, cfgs[i], sources, T) for i in ids}


def _restated(plan, attempt=0):
    """(mic, dp) int16 of the plan as the generator renders it at ``attempt``."""
    from sar_ssl_amd import roomsim
    n_len = roomsim.plan_rir(plan["cfg"])["n_len"]
    return roomsim.restate_sig(plan, roomsim.numpy_noise(SEED, plan["idx"], attempt, 2, n_len), with_dp=True)


def _against_restatement(name, wav, want):
    """The pass conditions of a written file (parity.SIMSIG: derived there, not measured here)."""
    from sar_ssl_amd import parity
    from sar_ssl_amd.dataset import read_wav_pcm16
    pcm, fs = read_wav_pcm16(wav)
    assert fs == sc.FS and pcm.shape == want.shape and pcm.dtype == np.int16
    d = np.abs(pcm.astype(np.int32) - want.astype(np.int32))
    print("PARITY %s.max_step measured=%d tol=%d (at most)" % (name, d.max(), parity.SIMSIG["pcm_step"]))
    assert d.max() <= parity.SIMSIG["pcm_step"], (name, int(d.max()))
    check(name + ".share", float((d != 0).mean()), parity.SIMSIG["share_bound"])
    return pcm


def _names(n, save_dp=True):
    return sorted(["%d%s" % (i, s) for i in range(n) for s in ((".wav", "_dp.wav", "_info.npz") if save_dp else (".wav", "_info.npz"))]
                  + ["all_info.npz"])


def _same_npz(fa, fb):
    ia, ib = np.load(fa, allow_pickle=True), np.load(fb, allow_pickle=True)
    return sorted(ia.files) == sorted(ib.files) and all(np.array_equal(ia[k], ib[k]) for k in ia.files)


@pytest.fixture(scope="module")
def e2e(tmp_path_factory, tree):
    tmp = tmp_path_factory.mktemp("sig_dp")
    res, lines = _simulate(tmp / "dp", tree, 3, 3)
    plain, _ = _simulate(tmp / "plain", tree, 3, 3, save_dp=False)
    one, _ = _simulate(tmp / "one", tree, 3, 1)
    return tmp, res, lines, plain, one


def test_save_dp_end_to_end_against_the_restatement(e2e, tree):
    from sar_ssl_amd import roomsim
    tmp, res, lines, plain, one = e2e
    out = tmp / "dp" / STAGE
    assert res["written"] == [0, 1, 2] and res["skipped"] == [] and lines == []
    assert sorted(os.listdir(out)) == _names(3)                       # (no .tmp left behind)
    plans = _plans(tree, range(3))
    for i in range(3):
        assert res["attempts"][i] <= roomsim.MAX_ATTEMPTS
        mic, dp = _restated(plans[i], res["attempts"][i] - 1)
        pm = _against_restatement("simsig_dp.idx%d.mic" % i, str(out / ("%d.wav" % i)), mic)
        pd = _against_restatement("simsig_dp.idx%d.dp" % i, str(out / ("%d_dp.wav" % i)), dp)
        assert max(np.abs(pm).max(), np.abs(pd).max()) >= 29000 and np.abs(pd).max() > 100     # mic or direct path sits at 0.9 of full scale
    args = np.load(out / "all_info.npz", allow_pickle=True)["args"].item()
    assert args["save_dp"] is True and args["stage"] == STAGE and args["seed"] == SEED


def test_save_dp_changes_nothing_else_that_is_written(e2e):
    tmp, res, lines, plain, one = e2e
    a, b = tmp / "dp" / STAGE, tmp / "plain" / STAGE
    assert plain == res and sorted(os.listdir(b)) == _names(3, save_dp=False)
    for i in range(3):
        assert (a / ("%d.wav" % i)).read_bytes() == (b / ("%d.wav" % i)).read_bytes()
        assert _same_npz(a / ("%d_info.npz" % i), b / ("%d_info.npz" % i))
    ia, ib = np.load(a / "all_info.npz", allow_pickle=True), np.load(b / "all_info.npz", allow_pickle=True)
    args_a, args_b = ia["args"].item(), ib["args"].item()
    assert "save_dp" not in args_b and {k: v for k, v in args_a.items() if k != "save_dp"}.keys() == args_b.keys()
    assert np.array_equal(ia["skipped"], ib["skipped"]) and len(ia["cfgs"]) == len(ib["cfgs"]) == 3


def test_save_dp_files_do_not_depend_on_the_batch(e2e):
    tmp, res, lines, plain, one = e2e
    a, b = tmp / "dp" / STAGE, tmp / "one" / STAGE
    assert one == res and sorted(os.listdir(b)) == _names(3)
    for i in range(3):
        for name in ("%d.wav" % i, "%d_dp.wav" % i):
            assert (a / name).read_bytes() == (b / name).read_bytes(), name
        assert _same_npz(a / ("%d_info.npz" % i), b / ("%d_info.npz" % i))


def test_save_dp_writes_both_files_of_a_retried_item_from_the_accepted_attempt(tmp_path, tree, monkeypatch):
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
    out = tmp_path / STAGE
    assert calls[0] == ([0, 1, 2], 0) and 1 in calls[1][0] and calls[1][1] == 1
    assert res["written"] == [0, 1, 2] and res["skipped"] == [] and res["attempts"][1] >= 2
    assert sorted(os.listdir(out)) == _names(3)
    plan = _plans(tree, [1])[1]
    mic, dp = _restated(plan, res["attempts"][1] - 1)
    pm = _against_restatement("simsig_dp.retry.mic", str(out / "1.wav"), mic)
    pd = _against_restatement("simsig_dp.retry.dp", str(out / "1_dp.wav"), dp)
    # the first attempt's RIR has another tail: its microphone signal is another one, and so is the divisor both files share
    mic0, dp0 = _restated(plan, 0)
    assert (np.abs(pm.astype(np.int32) - mic0) > 1).any()
    if (np.abs(dp.astype(np.int32) - dp0) > 2).any():
        assert (np.abs(pd.astype(np.int32) - dp0) > 1).any()


# ---------------------------------------------------------------------------------------------------------------- the product
def test_generated_corpus_feeds_the_instance_test(tmp_path, tree, monkeypatch):
    """gen_simu.py's pretest_ins_T1000 corpus with its direct-path files, then run_pretrain.py --test --test-mode ins over it."""
    import scipy.io
    import sar_ssl_amd.run_pretrain as rp
    from sar_ssl_amd import dataset, model, runtime
    work = tmp_path / "work"
    simu = work / "SAR-SSL" / "data" / "MicSig" / "simu"
    simu.mkdir(parents=True)
    res, lines = _simulate(simu, tree, 2, 2, T=4.112, noise="device")
    assert res["written"] == [0, 1] and sorted(os.listdir(simu / STAGE)) == _names(2)
    ck = work / "SAR-SSL" / "exp" / "pretrain" / "t3"
    ck.mkdir(parents=True)
    net = model.SARSSL(sig_shape=(256, 256, 2, 2), pretrain=True, device="cpu")
    torch.save({"epoch": 5, "max_score": -1.0, "model": net.state_dict()}, str(ck / "best_model.tar"))
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", os.environ.get("HIP_VISIBLE_DEVICES", "0"))       # (main sets it: restored afterwards)
    try:
        rp.main(["--test", "--test-mode", "ins", "--simu-exp", "--gpu-id", "0,", "--work-dir", str(work), "--bs", "4", "4", "4", "--workers", "0",
                 "--time", "t3", "--use-amp"])
    finally:
        runtime.set_precision("bf16")
    out = ck / "test_result"
    assert sorted(os.listdir(out)) == sorted(["rt1000_ins%d_epoch5_test_%s.wav" % (i, k) for i in (0, 1) for k in ("pred", "tar")]
                                             + ["rt1000_ins_epoch5_test.mat"])
    mat = scipy.io.loadmat(str(out / "rt1000_ins_epoch5_test.mat"))
    assert mat["pred"].shape == (2, 256, 256, 2, 2) and mat["mask"].shape == (2, 256, 256, 2)
    for i in (0, 1):
        pcm, fs = dataset.read_wav_pcm16(str(out / ("rt1000_ins%d_epoch5_test_tar.wav" % i)))
        assert fs == 16000 and pcm.shape == (65792, 2) and np.abs(pcm).max() > 1000
