"""GPU: the downstream test stage (``run_downstream.py --ds-test``) - ensemble checkpoint -> load_checkpoint_ensemble -> test_epoch against
the real reference's (fixture F19, tools/make_golden_dstest.py: TDOA at nt = 64 with 'spat', T60 at nt = 256 with 'spec_spat'), that the
captured evaluation step is what ran, a reference-layout ensemble file, and the three modes of the command line in a child process."""
import functools
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLD, ROOT, check

pytestmark = pytest.mark.gpu

PRECS = ["fp32", "bf16", "fp16", "hybrid"]
# The per-mode classes of tests/test_gpu_downstream.py (its TOL[prec]["epoch"] for an epoch's loss / metric, TOL[prec]["pred"] for
# max|embed - ref| / max|ref|), restated: that file is a GPU test module of its own and is not imported for two numbers.
CLASS = {"fp32": dict(epoch=2e-3, pred=2e-3), "bf16": dict(epoch=5e-2, pred=5e-2), "fp16": dict(epoch=2e-2, pred=2e-2),
         "hybrid": dict(epoch=2e-2, pred=5.9e-3)}
# T60 at nt = 256, 'spec_spat', eval mode: nobody had measured this shape, so each gate is 2.5x what was measured against F19 on an MI355X
# (the convention of tests/test_gpu_downstream.py; 'epoch' covers the loss and the metric: 2.5x the larger), never above the mode's class gate.
T60_TOL = {"fp32": dict(epoch=1.9e-5, pred=2.0e-5),        # measured: loss 7.4e-6, metric 4.2e-6, embed 7.8e-6
           "bf16": dict(epoch=7.0e-3, pred=1.0e-2),        # measured: loss 2.8e-3, metric 1.6e-3, embed 4.1e-3
           "fp16": dict(epoch=4.3e-4, pred=1.2e-3),        # measured: loss 1.7e-4, metric 7.1e-5, embed 4.7e-4
           "hybrid": dict(epoch=2.0e-4, pred=3.6e-4)}      # measured: loss 8.0e-5, metric 6.3e-5, embed 1.4e-4


@functools.lru_cache(maxsize=None)
def _gen():
    spec = importlib.util.spec_from_file_location("make_golden_dstest", os.path.join(ROOT, "tools", "make_golden_dstest.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def _f19():
    return dict(np.load(os.path.join(GOLD, "f19_dstest.npz"), allow_pickle=False))


@functools.lru_cache(maxsize=None)
def _case(name):
    """(case constants, its recipe states, its batches): built once, shared and left unchanged."""
    from sar_ssl_amd import model
    gen = _gen()
    c = getattr(gen, name)
    man = gen.manifest_of(gen.build_net(model, c, device="cpu"))
    return c, gen.states(man, c), gen.loader(c)


def _learner(c, prec):
    """A fresh model and learner of case ``c`` on the GPU in numeric mode ``prec``."""
    from sar_ssl_amd import learner, model, runtime
    net = _gen().build_net(model, c, device=torch.device("cuda:0"))
    lrn = learner.STFTLearner(net, win_len=512, win_shift_ratio=0.5, nfft=512, fre_used_ratio=1, fs=16000, task=c["task"], ch_mode="M")
    lrn.cuda()
    if prec != "fp32":
        lrn.amp(prec)
    else:
        runtime.set_precision("fp32")
    return net, lrn


@pytest.fixture(scope="module")
def ensemble_dir(tmp_path_factory):
    """model1.tar / model2.tar of the two TDOA recipe states, written with this build's save_checkpoint, and their ensembling([1, 2])."""
    from sar_ssl_amd import runtime
    c, sds, _ = _case("TDOA")
    d = str(tmp_path_factory.mktemp("dstest_ens"))
    try:
        net, lrn = _learner(c, "fp32")
        for epoch, sd in enumerate(sds, start=1):
            net.load_state_dict(sd)
            lrn.save_checkpoint(epoch=epoch, checkpoints_dir=d, is_best_epoch=False, save_extra_hist=True)
        lrn.ensembling(d, [1, 2])
    finally:
        runtime.set_precision("bf16")
    return d


def _rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


def _embed_err(vis, ref):
    e_ref = torch.from_numpy(ref)
    return float((vis["embed"].float().cpu() - e_ref).abs().max() / e_ref.abs().max())


def _check_epoch(tag, out, z, key, tol):
    loss, metric, vis = out
    ref = z[key + ".embed"]
    assert tuple(vis["embed"].shape) == ref.shape and tuple(vis["label"].shape) == (ref.shape[0], 1)
    assert torch.isfinite(vis["embed"].float()).all()
    np.testing.assert_allclose(vis["label"].float().cpu().numpy(), z[key + ".label"], rtol=1e-6)
    check(tag + ".loss", _rel(loss, z[key + ".loss"]), tol["epoch"])
    check(tag + ".metric", _rel(metric, z[key + ".metric"]), tol["epoch"])
    check(tag + ".embed", _embed_err(vis, ref), tol["pred"])


def _check_ensemble_sums(tag, net, z):
    sd = net.state_dict()
    for k in _gen().ENSEMBLE_KEYS:
        v = sd[k].double()
        short = k.rsplit(".", 1)[-1]
        check("%s.sum.%s" % (tag, short), _rel(v.sum(), z["tdoa.sum." + k]), 1e-6)
        check("%s.abssum.%s" % (tag, short), _rel(v.abs().sum(), z["tdoa.abssum." + k]), 1e-6)
    for k, v in sd.items():
        if k.endswith("num_batches_tracked"):
            assert v.dtype == torch.int64 and int(v) == 15, (k, v)


@pytest.mark.parametrize("prec", PRECS)
def test_tdoa_ensemble_test_epoch_vs_reference(prec, ensemble_dir):
    """37 segments at nt = 64 in batches of 16, 16 and 5 on a second, fresh learner that read ensemble_model.tar."""
    from sar_ssl_amd import runtime
    try:
        c, _, loader = _case("TDOA")
        net, lrn = _learner(c, prec)
        assert lrn.load_checkpoint_ensemble(ensemble_dir) == [1, 2]
        _check_ensemble_sums("dstest.tdoa.%s" % prec, net, _f19())
        _check_epoch("dstest.tdoa.%s" % prec, lrn.test_epoch(loader, True, True), _f19(), "tdoa", CLASS[prec])
    finally:
        runtime.set_precision("bf16")


@pytest.mark.parametrize("prec", PRECS)
def test_t60_spec_spat_test_epoch_vs_reference(prec):
    """7 segments at nt = 256 (the duration of the four non-TDOA tasks) in batches of 4 and 3, the head on both encoders' embeddings."""
    from sar_ssl_amd import runtime
    assert all(T60_TOL[prec][k] <= CLASS[prec][k] for k in ("epoch", "pred"))
    try:
        c, sds, loader = _case("T60")
        net, lrn = _learner(c, prec)
        lrn._load_model_state(sds[0], as_all_state=True)
        _check_epoch("dstest.t60.%s" % prec, lrn.test_epoch(loader, True, True), _f19(), "t60", T60_TOL[prec])
    finally:
        runtime.set_precision("bf16")


def test_the_replay_is_what_ran(ensemble_dir, monkeypatch):
    """Default switch: the two full batches are eval_step replays, the ragged tail of 5 takes eval_step_eager, nothing else runs."""
    from sar_ssl_amd import runtime
    from sar_ssl_amd.graph import DownstreamStepGraph
    monkeypatch.delenv("SARSSL_GRAPH", raising=False)
    try:
        c, _, loader = _case("TDOA")
        net, lrn = _learner(c, "hybrid")
        lrn.load_checkpoint_ensemble(ensemble_dir)
        assert "_step_graph" not in lrn.__dict__                            # the load dropped whatever was captured
        net.eval()
        g = lrn._downstream_graph()
        assert isinstance(g, DownstreamStepGraph)
        calls = {"eval_step": 0, "eval_step_eager": 0}
        for name in calls:
            def counted(*a, _f=getattr(g, name), _n=name, **k):
                calls[_n] += 1
                return _f(*a, **k)
            monkeypatch.setattr(g, name, counted, raising=True)
        out = lrn.test_epoch(loader, True, True)
        assert lrn.__dict__.get("_step_graph") is g and sorted(g._plans) == [False]
        assert calls == {"eval_step": 2, "eval_step_eager": 1}
        _check_epoch("dstest.replayed.hybrid", out, _f19(), "tdoa", CLASS["hybrid"])
    finally:
        runtime.set_precision("bf16")


@pytest.mark.parametrize("prec", ["fp32", "hybrid"])
def test_replayed_epoch_equals_launch_by_launch(prec, ensemble_dir, monkeypatch):
    """SARSSL_GRAPH=0 on the same learner: same loss, metric and embeddings, under the comparison of
    tests/test_gpu_downstream_graph.py::test_eval_replay_follows_the_trained_weights - hybrid: loss words to 1e-6, pooled embeddings bit
    for bit; fp32: 5e-4."""
    from sar_ssl_amd import runtime
    try:
        monkeypatch.setenv("SARSSL_GRAPH", "1")
        c, _, loader = _case("TDOA")
        net, lrn = _learner(c, prec)
        lrn.load_checkpoint_ensemble(ensemble_dir)
        l1, m1, v1 = lrn.test_epoch(loader, True, True)
        assert "_step_graph" in lrn.__dict__
        monkeypatch.setenv("SARSSL_GRAPH", "0")
        l2, m2, v2 = lrn.test_epoch(loader, True, True)
        gate = 1e-6 if prec == "hybrid" else 5e-4
        check("dstest.graph_vs_eager.%s.loss" % prec, _rel(l1, l2), gate)
        check("dstest.graph_vs_eager.%s.metric" % prec, _rel(m1, m2), gate)
        assert torch.equal(v1["label"].float(), v2["label"].float())
        if prec == "hybrid":
            assert torch.equal(v1["embed"].float(), v2["embed"].float())
        else:
            check("dstest.graph_vs_eager.fp32.embed", float((v1["embed"] - v2["embed"]).abs().max() / v2["embed"].abs().max()), 5e-4)
    finally:
        runtime.set_precision("bf16")


def test_reference_layout_ensemble_file_loads(ensemble_dir, tmp_path):
    """An ensemble file the way the reference's averaging leaves it - DataParallel's 'module.' key prefix, num_batches_tracked as float
    (long * 1/n), 'epoch' a list: the loaded model equals the one read from this build's file bit for bit, the counters are integers
    again, and the epoch gives the first case's numbers."""
    from sar_ssl_amd import runtime
    try:
        c, _, loader = _case("TDOA")
        own = torch.load(os.path.join(ensemble_dir, "ensemble_model.tar"), map_location="cpu", weights_only=False)
        sd = {"module." + k: (v.double().float() if k.endswith("num_batches_tracked") else v.clone()) for k, v in own["model"].items()}
        assert sd["module." + _gen().ENSEMBLE_KEYS[2]].dtype == torch.float32
        torch.save({"epoch": [1, 2], "model": sd}, str(tmp_path / "ensemble_model.tar"))
        net_a, lrn_a = _learner(c, "hybrid")
        lrn_a.load_checkpoint_ensemble(ensemble_dir)
        la, ma, va = lrn_a.test_epoch(loader, True, True)
        net_b, lrn_b = _learner(c, "hybrid")
        assert lrn_b.load_checkpoint_ensemble(str(tmp_path)) == [1, 2]
        sa, sb = net_a.state_dict(), net_b.state_dict()
        assert list(sa) == list(sb)
        for k in sa:
            assert sa[k].dtype == sb[k].dtype and torch.equal(sa[k], sb[k]), k
        _check_ensemble_sums("dstest.reflayout", net_b, _f19())
        out = lrn_b.test_epoch(loader, True, True)
        _check_epoch("dstest.reflayout.hybrid", out, _f19(), "tdoa", CLASS["hybrid"])
        assert out[0] == la and float(out[1]) == float(ma) and torch.equal(out[2]["embed"], va["embed"])
    finally:
        runtime.set_precision("bf16")


# ---- the command line, one child process per mode -------------------------------------------------------------------------------------
RUN = "finetune-all-mlp-8-0.0001-4-0-spat-sim_R32"
NSEL = 16640                                             # T = 1.04 s at 16 kHz


@pytest.fixture(scope="module")
def cli_tree(tmp_path_factory):
    """The directory tree of the entry-point test of tests/test_gpu_downstream.py (8 train / 4 val / 4 test WAV + _info.npz files) and an
    ensemble_model.tar of a recipe state in the run directory: no training."""
    from sar_ssl_amd import dataset, synth
    work = tmp_path_factory.mktemp("dstest_cli") / "work"
    rng = np.random.default_rng(3)
    for sub, n, base in (("train/R1", 8, 0), ("val", 4, 100), ("test", 4, 200)):
        d = work / "SAR-SSL" / "data" / "MicSig" / "simu_ds" / sub
        d.mkdir(parents=True)
        pcm = synth.to_pcm16(synth.make_batch(base, n))[:, :20000]
        for i in range(n):
            dataset.write_wav_pcm16(str(d / ("%d.wav" % i)), pcm[i])
            np.savez(str(d / ("%d_info.npz" % i)), TDOA=np.float64(rng.uniform(-5e-4, 5e-4)), T60_edc=np.float64(0.5), DRR=np.float64(1.0),
                     C50=np.float64(2.0), room_sz=np.array([4.0, 5.0, 3.0]))
    run = work / "SAR-SSL" / "exp" / "TDOA" / "t1" / RUN
    run.mkdir(parents=True)
    torch.save({"epoch": [1], "model": _case("TDOA")[1][0]}, str(run / "ensemble_model.tar"))
    return work


def _cli(work, mode):
    cmd = [sys.executable, os.path.join(ROOT, "run_downstream.py"), "--ds-test", "--simu-exp", "--test-mode", mode, "--ds-trainmode", "finetune",
           "--ds-task", "TDOA", "--ds-nsimroom", "32", "--ds-num", "8", "--ds-lr-set", "0.0001", "--ds-bs-set", "4", "--ds-eval-num", "4",
           "--workers", "2", "--gpu-id", "0,", "--work-dir", str(work), "--time", "t1"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    res = work / "SAR-SSL" / "exp" / "TDOA" / "t1" / "test_result"
    rec = json.load(open(res / ("%s-finetune.json" % mode)))
    assert rec["task"] == "TDOA" and rec["test_mode"] == mode and rec["lr"] == 0.0001 and rec["bs"] == 4
    assert len(rec["trials"]) == 1 and rec["trials"][0]["run"] == RUN
    return res, rec, r.stdout


def _datasets(work):
    from sar_ssl_amd import dataset
    base = work / "SAR-SSL" / "data" / "MicSig" / "simu_ds"
    sel = dataset.Selecting(select_range=[0, NSEL])
    # (a list of directories is shuffled with numpy's global generator: only order-free properties of the training set are compared)
    train =dataset.FixMicSigDataset(data_dir=[str(base / "train" / "R1")], load_anno=True, load_dp=False, fs=16000, dataset_sz=8, transforms=[sel])
    test = dataset.FixMicSigDataset(data_dir=str(base / "test"), load_anno=True, load_dp=False, fs=16000, dataset_sz=4, transforms=[sel])
    return train, test


def _tdoa_of(ds):
    return np.array([float(np.load(str(f).replace(".wav", "_info.npz"))["TDOA"]) for f in ds.files[:len(ds)]], dtype=np.float32)


def test_cli_cal_metric(cli_tree):
    from sar_ssl_amd import runtime
    from sar_ssl_amd.common.utils import set_random_seed
    res, rec, out = _cli(cli_tree, "cal_metric")
    assert "TDOA estimation, Test loss:" in out
    try:
        c = _case("TDOA")[0]
        net, lrn = _learner(c, "fp32")                   # (no --use-amp)
        lrn.load_checkpoint_ensemble(str(cli_tree / "SAR-SSL" / "exp" / "TDOA" / "t1" / RUN))
        dl = torch.utils.data.DataLoader(_datasets(cli_tree)[1], batch_size=16, shuffle=False)
        set_random_seed(2)                               # seeds["test"] = --seed + 1
        loss, metric = lrn.test_epoch(dl, return_metric=True)
    finally:
        runtime.set_precision("bf16")
    t = rec["trials"][0]
    assert t["epochs"] == [1] and np.isfinite(t["loss"]) and np.isfinite(t["metric"])
    check("dstest.cli.cal_metric.loss", _rel(t["loss"], loss), 1e-6)
    check("dstest.cli.cal_metric.metric", _rel(t["metric"], metric), 1e-6)
    assert rec["mean"]["loss"] == t["loss"] and rec["mean"]["metric"] == t["metric"]


def test_cli_cal_metric_wo_info(cli_tree):
    res, rec, out = _cli(cli_tree, "cal_metric_wo_info")
    train, test = _datasets(cli_tree)
    gt, gt_test = _tdoa_of(train)[:, None] * np.float32(16000), _tdoa_of(test)[:, None] * np.float32(16000)
    mean = float(gt.mean(dtype=np.float32))
    want = {"mae_test": float(np.abs(gt_test - np.float32(mean)).mean(dtype=np.float32)), "min_test": float(gt_test.min()),
            "max_test": float(gt_test.max()), "mae_train": float(np.abs(gt - np.float32(mean)).mean(dtype=np.float32)), "mean_train": mean,
            "min_train": float(gt.min()), "max_train": float(gt.max())}
    t = rec["trials"][0]
    for k, v in want.items():                            # f32 sums of 8 / 4 values in another order: a few ulps
        assert abs(t[k] - v) <= 1e-5 * abs(v), (k, t[k], v)
        assert rec["mean"][k] == t[k]
    assert "Data MAE:" in out


def test_cli_vis_embed(cli_tree):
    import scipy.io
    res, rec, out = _cli(cli_tree, "vis_embed")
    train, test = _datasets(cli_tree)
    te = scipy.io.loadmat(str(res / ("embed_test_%s.mat" % RUN)))
    tr = scipy.io.loadmat(str(res / ("embed_train_%s.mat" % RUN)))
    assert te["embed"].shape == (4, 256) and te["embed"].dtype == np.float32 and np.isfinite(te["embed"]).all()
    assert tr["embed"].shape == (8, 256) and np.isfinite(tr["embed"]).all() and tr["label"].shape == (8, 1)
    np.testing.assert_allclose(te["label"], _tdoa_of(test)[:, None] * np.float32(16000), rtol=1e-6)
    try:
        import sklearn.manifold  # noqa: F401
        import matplotlib  # noqa: F401
        have = True
    except ImportError:
        have = False
    for stage, n in (("train", 8), ("test", 4)):
        for ext in (".png", ".mat"):
            assert (res / ("tsne_vis_%s_%s%s" % (stage, RUN, ext))).exists() == have
        if have:
            m = scipy.io.loadmat(str(res / ("tsne_vis_%s_%s.mat" % (stage, RUN))))
            assert m["data"].shape == (n, 2) and np.isfinite(m["data"]).all()
    assert np.isfinite(rec["trials"][0]["loss"]) and np.isfinite(rec["trials"][0]["loss_train"])
