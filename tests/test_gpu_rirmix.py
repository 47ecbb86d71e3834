"""GPU: the RIR renderer (csrc/rirmix.hip: sarssl_rir_mix, sarssl_diffuse_noise, sarssl_gauss_fill) against the f64 numpy / scipy
restatement of one item (sar_ssl_amd/rirsynth.py), on the smallest shapes that can still go wrong; the loader over the reference's fixture
F20; one train / test epoch fed by it; the command line without --simu-exp.

All outputs are peak-normalised, so an absolute error is an error relative to full scale.  Gate: parity.RIRMIX["gate"] (4x the largest
distance measured on an MI355X over the shapes below, one digit, see profiles/rirmix.txt), never above the hard cap of 1.5e-5 = half a
PCM-16 step."""
import functools
import math

import numpy as np
import pytest
import torch

from conftest import check

pytestmark = pytest.mark.gpu

N0 = 40
SNRS = (-5.0, 0.0, 30.0)


def _gate():
    from sar_ssl_amd import parity
    assert parity.RIRMIX["gate"] <= parity.RIRMIX["cap"] == 1.5e-5
    return parity.RIRMIX["gate"]


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def _render(items, nch, explicit, with_noise=True):
    """items: dicts of src (Ns,), rir (nch, L), [rir_dp (nch, Ld)], noise (Ns, nch), snr, gain -> GPU output (B, Ns, nch) as numpy."""
    from sar_ssl_amd import hip
    B, Ns = len(items), items[0]["src"].shape[0]
    Lmax = max(it["rir"].shape[1] for it in items)
    rir = np.zeros((B, nch, Lmax), np.float32)
    for b, it in enumerate(items):
        rir[b, :, :it["rir"].shape[1]] = it["rir"]
        rir[b, :, it["rir"].shape[1]:] = 7.0        # past rir_len: must never be read as signal (nor win the argmax)
    kw = {}
    if explicit:
        Ld = max(it["rir_dp"].shape[1] for it in items)
        dp = np.full((B, nch, Ld), 7.0, np.float32)
        for b, it in enumerate(items):
            dp[b, :, :it["rir_dp"].shape[1]] = it["rir_dp"]
        kw = dict(rir_dp=_dev(dp), dp_len=_dev(np.array([it["rir_dp"].shape[1] for it in items]), torch.int32))
    else:
        kw = dict(n0=N0)
    noise = _dev(np.stack([it["noise"] for it in items])) if with_noise else None
    out = hip.rir_mix(_dev(np.stack([it["src"] for it in items])), _dev(rir),
                      _dev(np.array([it["rir"].shape[1] for it in items]), torch.int32),
                      _dev(np.array([it["snr"] for it in items])), _dev(np.array([it["gain"] for it in items])), noise=noise, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _restate(it, explicit, with_noise=True):
    from sar_ssl_amd import rirsynth
    return rirsynth.restate_mix(it["src"], it["rir"], rir_dp=it["rir_dp"] if explicit else None, n0=None if explicit else N0,
                                noise=it["noise"] if with_noise else None, snr_db=it["snr"], gain=it["gain"])


def _item(rs, Ns, L, nch, snr=0.0, gain=0.9, Ld=None):
    rir = (rs.standard_normal((nch, L)) * np.exp(-np.arange(L) / max(L / 4.0, 1.0))).astype(np.float32)
    Ld = min(L, 64) if Ld is None else Ld
    return dict(src=rs.standard_normal(Ns).astype(np.float32), rir=rir, rir_dp=rir[:, :Ld].copy() * np.float32(0.5),
                noise=rs.standard_normal((Ns, nch)).astype(np.float32), snr=snr, gain=gain)


def _worst(out, items, explicit, with_noise=True):
    return max(float(np.abs(out[b] - _restate(it, explicit, with_noise)).max()) for b, it in enumerate(items))


@pytest.mark.parametrize("nch", [1, 2, 3])
@pytest.mark.parametrize("Ns", [256, 1000, 4352])
def test_rir_mix_lengths(Ns, nch):
    """One ragged batch per (Ns, nch): L = 1, 255, 256, 257, 700 and one L > Ns, with explicit and with windowed direct paths."""
    rs = np.random.RandomState(1000 * nch + Ns)
    Ls = [1, 255, 256, 257, 700, Ns + 300]
    items = [_item(rs, Ns, L, nch, snr=SNRS[i % 3], gain=(0.9, 1.0)[i % 2]) for i, L in enumerate(Ls)]
    worst = max(_worst(_render(items, nch, True), items, True), _worst(_render(items, nch, False), items, False))
    check("rir_mix Ns=%d nch=%d" % (Ns, nch), worst, _gate())


def test_rir_mix_delta_is_the_source():
    rs = np.random.RandomState(5)
    it = _item(rs, 1000, 1, 2)
    it["rir"][:] = 1.0
    it["rir_dp"] = it["rir"].copy()
    out = _render([it], 2, True, with_noise=False)[0]
    want = it["src"].astype(np.float64) / np.abs(it["src"]).max() * 0.9
    check("rir_mix delta", np.abs(out - want[:, None]).max(), _gate())
    check("rir_mix delta vs restatement", _worst(out[None], [it], True, False), _gate())


def test_rir_mix_ragged_batch_of_three():
    rs = np.random.RandomState(6)
    items = [_item(rs, 1000, L, 2, snr=s, Ld=Ld) for L, Ld, s in ((300, 17, -5.0), (513, 300, 0.0), (900, 1, 30.0))]
    check("rir_mix ragged explicit", _worst(_render(items, 2, True), items, True), _gate())
    check("rir_mix ragged window", _worst(_render(items, 2, False), items, False), _gate())


def _peaked(rs, L, nch, peaks):
    """Small decaying noise with the given (index, value) peaks per channel."""
    rir = (0.05 * rs.standard_normal((nch, L)) * np.exp(-np.arange(L) / 200.0)).astype(np.float32)
    for c in range(nch):
        for i, v in peaks[c % len(peaks)]:
            rir[c, i] = v
    return rir


@pytest.mark.parametrize("case", ["clipped_at_0", "straddles_partition", "near_end", "tie_first_wins", "signed_maximum"])
def test_rir_mix_windowed_direct_path(case):
    L, Ns, nch = 700, 1000, 2
    rs = np.random.RandomState(7)
    peaks = {"clipped_at_0": [[(5, 1.0)], [(9, 0.8)]],
             "straddles_partition": [[(250, 1.0)], [(262, 0.7)]],
             "near_end": [[(L - 3, 1.0)], [(L - 1, 0.9)]],
             "tie_first_wins": [[(100, 1.0), (400, 1.0)], [(300, 0.5), (301, 0.5)]],
             "signed_maximum": [[(100, -2.0), (300, 1.0)], [(50, -3.0), (520, 0.25)]]}[case]
    items = []
    for snr in SNRS:
        it = _item(rs, Ns, L, nch, snr=snr)
        it["rir"] = _peaked(rs, L, nch, peaks)
        items.append(it)
    from sar_ssl_amd import rirsynth
    nd = np.argmax(items[0]["rir"], axis=1)
    assert list(nd) == [p[0][0] if case != "signed_maximum" else p[1][0] for p in peaks], nd
    assert np.count_nonzero(rirsynth.direct_path_window(items[0]["rir"], N0)[0]) <= 2 * N0 + 1
    check("rir_mix window " + case, _worst(_render(items, nch, False), items, False), _gate())


def test_rir_mix_negative_peak_and_null_noise():
    rs = np.random.RandomState(8)
    items = [_item(rs, 1000, 257, 2, snr=s) for s in SNRS]
    for it in items:
        it["src"][137] = -40.0                    # the output's largest magnitude is a negative sample
        it["rir"][:, 0], it["rir_dp"][:, 0] = 10.0, 5.0
    out = _render(items, 2, True, with_noise=False)
    for b, it in enumerate(items):
        want = _restate(it, True, False)
        assert want.min() == pytest.approx(-0.9, abs=1e-12) and want.max() < 0.9
        assert out[b].min() == pytest.approx(-0.9, abs=1e-6)
    check("rir_mix null noise, negative peak", _worst(out, items, True, False), _gate())
    out = _render(items, 2, True, with_noise=True)
    check("rir_mix negative peak with noise", _worst(out, items, True, True), _gate())


# ---------------------------------------------------------------------------------------------------------------- diffuse field
def _mic_pos(rs, M):
    return rs.uniform(-0.1, 0.1, size=(M, 3))


@pytest.mark.parametrize("M", [2, 4])
@pytest.mark.parametrize("Ns", [64, 4352])
def test_diffuse_noise_vs_scipy(Ns, M):
    from sar_ssl_amd import hip, rirsynth
    rs = np.random.RandomState(10 * M + Ns)
    B = 2
    white = rs.standard_normal((B, Ns, M)).astype(np.float32)
    C = np.stack([rirsynth.mixing_table(_mic_pos(rs, M)) for _ in range(B)])
    assert np.all(C[:, 0] == 0) and np.all(np.tril(C[:, 5], -1) == 0)
    out = hip.diffuse_noise(_dev(white), _dev(C))
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    C32 = C.astype(np.float32).astype(np.float64)
    worst = max(float(np.abs(out[b] - rirsynth.restate_diffuse(white[b], C32[b])).max()) for b in range(B))
    check("diffuse_noise Ns=%d M=%d" % (Ns, M), worst, _gate())


def test_diffuse_noise_refuses_other_lengths():
    from sar_ssl_amd import _lib, hip, rirsynth
    white = torch.randn(1, 100, 2, device="cuda")
    C = _dev(rirsynth.mixing_table(np.array([[0, 0, 0], [0.08, 0, 0]], float))[None])
    out = torch.full_like(white, 3.0)
    with pytest.raises(_lib.SarsslHipError, match="64"):
        hip.diffuse_noise(white, C, out=out)
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())


# ---------------------------------------------------------------------------------------------------------------- Gaussian fill
def test_gauss_fill_is_a_function_of_its_key():
    from sar_ssl_amd import hip
    a = hip.gauss_fill(torch.empty(3, 1001, 3, device="cuda"), seed=1234, item0=5)
    b = hip.gauss_fill(torch.empty(3, 1001, 3, device="cuda"), seed=1234, item0=5)
    c = hip.gauss_fill(torch.empty(3, 1001, 3, device="cuda"), seed=1234, item0=6)
    d = hip.gauss_fill(torch.empty(3, 1001, 3, device="cuda"), seed=1235, item0=5)
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    assert torch.equal(a[1:], c[:2])                       # item index = item0 + b
    assert not torch.equal(a[0], c[0]) and not torch.equal(a, d)
    assert float((a[0] == a[1]).float().mean()) < 0.01


def test_gauss_fill_moments():
    """N = 2^20 values: the sample mean has standard deviation 1/sqrt(N), the sample variance sqrt(2/N); both gated at 5 sigma."""
    from sar_ssl_amd import hip
    N = 1 << 20
    x = hip.gauss_fill(torch.empty(1, N // 2, 2, device="cuda"), seed=99).double().flatten()
    mean, var = float(x.mean()), float(x.var(unbiased=True))
    print("gauss_fill mean=%.3e var-1=%.3e" % (mean, var - 1))
    assert abs(mean) < 5 / math.sqrt(N)
    assert abs(var - 1) < 5 * math.sqrt(2.0 / N)


def test_gauss_fill_through_the_diffuse_field_has_the_sinc_coherence():
    """Two microphones 8 cm apart, Ns = 65 536.  Coherence estimate Re(S12) / sqrt(S11 S22) from K non-overlapping-by-a-frame Hann-256
    snapshots (hop 512: independent, the field's own synthesis window is 256 long).  For K independent circular Gaussian snapshot pairs
    with real coherence g the delta method gives Var(Re g^) = (1 - g^2)^2 / (2K); the gate is 5 of these standard errors."""
    import scipy.signal
    from sar_ssl_amd import hip, rirsynth
    Ns, d, c = 65536, 0.08, 343.0
    white = hip.gauss_fill(torch.empty(1, Ns, 2, device="cuda"), seed=7)
    C = rirsynth.mixing_table(np.array([[0, 0, 0], [d, 0, 0]], float), c=c)
    y = hip.diffuse_noise(white, _dev(C[None]))[0].double().cpu().numpy()
    _, _, Y = scipy.signal.stft(y.T, window="hann", nperseg=256, noverlap=0, nfft=256, boundary=None, padded=False)
    Y = Y[:, :, ::2]
    K = Y.shape[2]
    assert K == 128
    for k in (8, 32, 96):
        s12 = np.sum(Y[0, k] * np.conj(Y[1, k]))
        est = float(np.real(s12) / math.sqrt(np.sum(np.abs(Y[0, k]) ** 2) * np.sum(np.abs(Y[1, k]) ** 2)))
        target = float(np.sinc(2 * math.pi * 16000 * k / 256 * d / (c * math.pi)))
        se = (1 - target ** 2) / math.sqrt(2 * K)
        print("coherence bin %d: estimate %.4f target %.4f se %.4f" % (k, est, target, se))
        assert abs(est - target) < 5 * se


# ---------------------------------------------------------------------------------------------------------------- loader, epochs, command line
@functools.lru_cache(maxsize=None)
def _gen():
    import importlib.util
    import os
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("make_golden_rirmix", os.path.join(ROOT, "tools", "make_golden_rirmix.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def _f20():
    import os
    from conftest import GOLD
    return dict(np.load(os.path.join(GOLD, "f20_rirmix.npz"), allow_pickle=False))


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """Fixture F20's tree on disk and the banks over it (sorted listings, as the fixture was made)."""
    from sar_ssl_amd import rirsynth
    gen = _gen()
    root = gen.restore_tree(str(tmp_path_factory.mktemp("f20_tree")), _f20())
    d = gen.dirs_of(root)
    return dict(measured=rirsynth.MeasuredBank(d["real_rooms"], fs=gen.FS, sort=True),
                simulated=rirsynth.SimulatedBank([d["rir_train_simu"]], fs=gen.FS, c=gen.C, sort=True),
                sources=rirsynth.SourceBank(d["src"], fs=gen.FS, sort=True))


def _loader(tree, n, bs, noise, ratio=(1, 1)):
    from sar_ssl_amd import rirsynth
    gen = _gen()
    return rirsynth.RirSynthLoader(tree["measured"], tree["simulated"], tree["sources"], dataset_sz=n, batch_size=bs, T=gen.T, fs=gen.FS,
                                   nmic=gen.NMIC, snr_range=gen.SNR_RANGE, real_sim_ratio=ratio, seed=gen.SEED, noise=noise, device="cuda:0", c=gen.C)


def test_loader_reproduces_the_reference_items(tree):
    """noise="numpy": the six consecutive RandomMicSigFromRIRDataset items of F20 (both variants, one full and one ragged batch), and
    its items by index rendered as one mixed batch - against the f64 restatement of the same plans (the gate) and against the reference's
    own outputs (the gate + the restatement's distance to them)."""
    from sar_ssl_amd import parity, rirsynth
    gen, f = _gen(), _f20()
    ld = _loader(tree, gen.OUTER_ITEMS, 4, "numpy")
    assert len(ld) == 2
    np.random.seed(gen.OUTER_SEED)
    plans = [p for b in ld.plan_batches() for p in b]
    np.random.seed(gen.OUTER_SEED)
    batches = list(ld)
    torch.cuda.synchronize()
    assert [tuple(b[0].shape) for b in batches] == [(4, gen.NS, 2), (2, gen.NS, 2)] and all(b[0].is_cuda and b[0].dtype == torch.float32 for b in batches)
    out = torch.cat([b[0] for b in batches]).cpu().numpy()
    labels = {k: torch.cat([b[1][k] for b in batches]).cpu().numpy() for k in ("T60", "DRR", "C50", "ABS")}
    d_res = max(float(np.abs(out[i] - rirsynth.restate_item(plans[i], tree["measured"], tree["simulated"], fs=gen.FS, c=gen.C)).max()) for i in range(gen.OUTER_ITEMS))
    d_ref = max(float(np.abs(out[i] - f["outer/%d/out" % i]).max()) for i in range(gen.OUTER_ITEMS))
    for k, v in labels.items():
        assert v.dtype == np.float32 and np.array_equal(v, np.array([f["outer/%d/label_%s" % (i, k)] for i in range(gen.OUTER_ITEMS)])), k
    check("loader outer items vs restatement", d_res, _gate())
    check("loader outer items vs F20", d_ref, _gate() + parity.RIRMIX["restatement_vs_f20"])

    kw = dict(T=gen.T, fs=gen.FS, snr_range=gen.SNR_RANGE)
    pre, plans = [], []
    for j in range(gen.ITEMS):
        plans.append(rirsynth.plan_measured(np.random.RandomState(0), int(f["measured_ids"][j]), gen.SEED, tree["measured"], tree["sources"], **kw))
        plans.append(rirsynth.plan_simulated(np.random.RandomState(0), int(f["simulated_ids"][j]), gen.SEED, tree["simulated"], tree["sources"], nmic=gen.NMIC, **kw))
        pre += ["measured/%d/" % j, "simulated/%d/" % j]
    sig, lab = ld.render(ld.host_batch(plans))
    torch.cuda.synchronize()
    sig = sig.cpu().numpy()
    check("loader items by index vs F20", max(float(np.abs(sig[i] - f[p + "out"]).max()) for i, p in enumerate(pre)),
          _gate() + parity.RIRMIX["restatement_vs_f20"])
    assert np.array_equal(lab["T60"].cpu().numpy(), np.array([f[p + "label_T60"] for p in pre]))


def test_train_and_test_epoch_fed_by_the_loader(tree):
    """One train_epoch and one test_epoch of a T = 0.272 s (nt = 16) downstream model on 2-batch loaders in noise="device" mode: finite loss
    and metric, bit-identical when repeated with the same seeds."""
    from sar_ssl_amd import learner, model, runtime
    from sar_ssl_amd.common.utils import set_seed
    gen = _gen()
    nt = int((gen.T * gen.FS - 256) / 256)
    assert nt == 16

    def once():
        set_seed(5)
        net = model.SARSSL(sig_shape=(256, nt, 2, 2), pretrain=False, device=torch.device("cuda:0"), downstream_token="all", downstream_head="mlp",
                           downstream_embed="spat", downstream_dlabel=1)
        lrn = learner.STFTLearner(net, win_len=512, win_shift_ratio=0.5, nfft=512, fre_used_ratio=1, fs=gen.FS, task="T60", ch_mode="M")
        lrn.cuda()
        runtime.set_precision("fp32")
        set_seed(11)
        tr = lrn.train_epoch(_loader(tree, 16, 8, "device"), lr=1e-4, epoch=1, return_metric=True)
        set_seed(12)
        te = lrn.test_epoch(_loader(tree, 16, 8, "device", ratio=(1, 0)), return_metric=True)
        return [float(tr[0]), float(tr[1]), float(te[0]), float(te[1])]

    import gc
    try:
        a, b = once(), once()
    finally:
        runtime.set_precision("bf16")                        # the suite's resting mode
        gc.collect()                                         # the two learners' captured steps are released here, not inside a later test
        torch.cuda.synchronize()
    print("train loss / metric, test loss / metric:", a)
    assert all(np.isfinite(a)) and a == b


def test_loader_device_noise_is_reproducible_and_differs_from_numpy(tree):
    gen = _gen()
    outs = []
    for noise in ("device", "device", "numpy"):
        np.random.seed(3)
        outs.append(torch.cat([b[0] for b in _loader(tree, 6, 4, noise, ratio=(0, 1))]))
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], outs[2])
    assert bool(torch.isfinite(outs[0]).all()) and float(outs[0].abs().max()) == pytest.approx(1.0, abs=1e-6)


def test_run_downstream_real_data_command_line(tmp_path):
    """`run_downstream.py --ds-train --ds-trainmode finetune --ds-task T60 --ds-real-sim-ratio 1 1` on a generated tree: one run directory per
    cross-validation trial (= room) and the result file with ntrial = the room count."""
    import json
    import os
    import shutil
    import subprocess
    import sys
    import scipy.io
    from conftest import ROOT
    from sar_ssl_amd import model
    gen = _gen()
    work = tmp_path / "work"
    rir_root = work / "SAR-SSL" / "data" / "RIR"
    gen.write_tree(str(rir_root), gen.tree_arrays(ns=int(4.112 * gen.FS)))
    for sub in ("tr", "dt", "et"):
        shutil.copytree(str(rir_root / "src" / "tr"), str(work / "data" / "SrcSig" / "wsj0" / sub))
    pre = model.SARSSL(sig_shape=(256, 256, 2, 2), pretrain=True, device="cpu")
    ck = work / "SAR-SSL" / "exp" / "pretrain" / "t1"
    ck.mkdir(parents=True)
    torch.save({"epoch": 3, "max_score": -1.0, "model": pre.state_dict()}, str(ck / "best_model.tar"))
    cmd = [sys.executable, os.path.join(ROOT, "run_downstream.py"), "--ds-train", "--ds-trainmode", "finetune", "--ds-task", "T60",
           "--ds-real-sim-ratio", "1", "1", "--gpu-id", "0,", "--work-dir", str(work), "--time", "t1", "--ds-nepoch", "1", "--ds-num", "16",
           "--ds-eval-num", "16", "--ds-lr-set", "0.001", "--ds-bs-set", "8"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    tdir = work / "SAR-SSL" / "exp" / "T60" / "t1"
    runs = sorted(p.name for p in tdir.iterdir() if p.is_dir())
    assert runs == ["finetune-all-mlp-16-0.001-8-%d-spat-real_train1real1sim_valreal" % t for t in range(len(gen.ROOMS))]
    for run in runs:
        recs = [json.loads(l) for l in open(tdir / run / "scalars.jsonl").read().strip().splitlines()]
        assert [r_["epoch"] for r_ in recs] == [1] and all(np.isfinite(r_[k]) for r_ in recs for k in ("loss_train", "loss_val", "metric_test"))
        assert (tdir / run / "ensemble_model.tar").exists()
    mats = [p for p in tdir.iterdir() if p.name.endswith("-lr_bs_tri_result.mat")]
    assert len(mats) == 1
    res = scipy.io.loadmat(str(mats[0]))
    assert int(res["ntrial"].squeeze()) == len(gen.ROOMS) and res["val_metrics"].shape == (1, 1, len(gen.ROOMS)) and np.isfinite(res["test_metrics"]).all()
