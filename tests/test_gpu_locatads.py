"""GPU: the device side of the LOCATA TDOA corpus - sarssl_interp_mean (hip.interp_mean) against np.interp(...).mean in f64 and
sarssl_peak_scale (hip.peak_scale) against numpy in f32 (csrc/locata.hip; gates in parity.LOCATADS), and locatads.generate on the
synthetic tree of tests/locatads_cases.py against locatads.TdoaCorpus.restate_item.

interp_mean: a ragged batch of five tables - one node, two nodes, 700 nodes (longer than the workgroup), one wholly behind the sample
times and one wholly ahead of them - at n = 1, 255, 256, 257 (a run of one or two samples per thread, threads without any) and 16 640,
with 1 and 8 columns; B = 1 with samples exactly on the nodes, the last one included.  Every output tensor is filled with NaN before
the call: an element the kernel leaves out fails the comparison."""
import os

import numpy as np
import pytest
import torch

from conftest import check

import locatads_cases as cases

pytestmark = pytest.mark.gpu
_REF = {}                          # computed once, left unchanged


def _tables(ncol):
    """[(ts, val (npoint, ncol), t0, dt)] of the five items."""
    if ncol not in _REF:
        rs = np.random.RandomState(270 + ncol)
        items = []
        for npoint, t0, dt in ((1, 0.0, 1.0 / 16000), (2, 0.13, 1.0 / 16000), (700, 0.37, 1.0 / 16000), (9, -40.0, 1.0 / 16000), (9, 55.0, 1.0 / 16000)):
            ts = np.cumsum(rs.uniform(0.2, 1.8, npoint)) * (2.0 / npoint)                        # irregular stamps over about 2 s
            val = rs.standard_normal((npoint, ncol)) * 2e-4
            for a in (ts, val):
                a.setflags(write=False)
            items.append((ts, val, t0, dt))
        _REF[ncol] = items
    return _REF[ncol]


def _want(item, n):
    ts, val, t0, dt = item
    t = t0 + np.arange(n) * dt
    return np.array([np.interp(t, ts, val[:, c]).mean() for c in range(val.shape[1])])


def _run(items, n, out=None):
    from sar_ssl_amd import hip
    off = np.concatenate(([0], np.cumsum([it[0].shape[0] for it in items]))).astype(np.int32)
    ts = torch.from_numpy(np.concatenate([it[0] for it in items])).cuda()
    val = torch.from_numpy(np.concatenate([it[1] for it in items])).cuda()
    ns = n if isinstance(n, (list, tuple)) else [n] * len(items)
    if out is None:
        out = torch.full((len(items), val.shape[1]), float("nan"), dtype=torch.float64, device="cuda")
    got = hip.interp_mean(off, ts, val, [it[2] for it in items], [it[3] for it in items], ns, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    return out.cpu().numpy()


def _units(got, want, val, n):
    """|got - want| in units of 2^-52 log2(max(n, 2)) of the column's largest |value|."""
    return float((np.abs(got - want) / (np.abs(val).max(axis=0) * 2.0 ** -52 * np.log2(max(n, 2)))).max())


@pytest.mark.parametrize("ncol", (1, 8))
@pytest.mark.parametrize("n", (1, 255, 256, 257, 16640))
def test_interp_mean_ragged_batch(n, ncol):
    from sar_ssl_amd import parity
    items = _tables(ncol)
    got = _run(items, n)
    worst = 0.0
    for b, it in enumerate(items):
        want = _want(it, n)
        if b >= 3 and n == 1:                                                                   # clamped: the end value itself
            assert np.array_equal(got[b], it[1][0 if b == 3 else -1]), b
        worst = max(worst, _units(got[b], want, it[1], n))
    check("interp_mean[n=%d,ncol=%d] (units of 2^-52 log2 n)" % (n, ncol), worst, parity.LOCATADS["interp_mean"]["ulps"])
    # the 700-node item alone: the same bits at another place of another batch, and on a second run
    alone = _run([items[2]], n)
    assert np.array_equal(alone[0].view(np.uint64), got[2].view(np.uint64))
    assert np.array_equal(_run(items, n).view(np.uint64), got.view(np.uint64))


def test_interp_mean_samples_on_the_nodes_and_mixed_lengths():
    from sar_ssl_amd import parity
    ts = np.array([0.0, 0.5, 1.0, 2.0])
    val = np.array([[1.0, -3.0], [2.0, 0.125], [-7.0, 0.3], [0.1, 11.0]])
    it = (ts, val, 0.0, 0.25)                                                                    # k / 4: every node is a sample, the last one too
    got = _run([it], 9)
    want = _want(it, 9)
    check("interp_mean[on nodes]", _units(got[0], want, val, 9), parity.LOCATADS["interp_mean"]["ulps"])
    for k, node in ((1, 0), (3, 1), (5, 2), (9, 3)):                                             # n = k: the mean's last sample sits on `node`
        one = _run([(ts, val, 0.25 * (k - 1), 0.25)], 1)
        assert np.array_equal(one[0], val[node]), (k, node)                                       # the node's value, unchanged
    still = (ts, val, 0.75, 0.0)                                                                 # dt = 0: one time, five times
    check("interp_mean[dt=0]", _units(_run([still], 5)[0], _want(still, 5), val, 5), parity.LOCATADS["interp_mean"]["ulps"])
    # every item its own n
    items = _tables(1)
    ns = [3, 16640, 257, 1, 255]
    got = _run(items, ns)
    for b, (item, n) in enumerate(zip(items, ns)):
        check("interp_mean[mixed n, item %d]" % b, _units(got[b], _want(item, n), item[1], n), parity.LOCATADS["interp_mean"]["ulps"])


def test_interp_mean_refusals_leave_out_untouched():
    from sar_ssl_amd import _lib, hip
    items = _tables(1)
    ts = torch.from_numpy(np.concatenate([it[0] for it in items])).cuda()
    val = torch.from_numpy(np.concatenate([it[1] for it in items])).cuda()
    off = np.concatenate(([0], np.cumsum([it[0].shape[0] for it in items]))).astype(np.int32)
    B = len(items)
    t0, dt, n = [0.0] * B, [1e-4] * B, [16] * B

    def refused(off=off, ts=ts, val=val, t0=t0, dt=dt, n=n, nb=B, ncol=1):
        out = torch.full((nb, ncol), 777.0, dtype=torch.float64, device="cuda")
        with pytest.raises(_lib.SarsslHipError):
            hip.interp_mean(off, ts, val, t0, dt, n, out=out)
        torch.cuda.synchronize()
        assert bool((out == 777.0).all())

    empty = off.copy()
    empty[2] = empty[1]                                                                          # npoint < 1
    refused(off=empty)
    refused(n=[16, 16, 0, 16, 16])                                                               # n < 1
    refused(val=torch.zeros((ts.shape[0], 9), dtype=torch.float64, device="cuda"), ncol=9)       # ncol > 8
    refused(dt=[1e-4, -1e-4, 1e-4, 1e-4, 1e-4])
    refused(t0=[0.0, float("nan"), 0.0, 0.0, 0.0])
    short = off.copy()
    short[-1] -= 1                                                                               # offsets that do not end at ntotal
    refused(off=short)
    lib = _lib.lib()                                                                             # B > 65535: by the entry point itself
    big = np.arange(65537 + 1, dtype=np.int32)
    z, ones = np.zeros(65537), np.ones(65537, np.int32)
    out = torch.full((4,), 777.0, dtype=torch.float64, device="cuda")
    rc = lib.sarssl_interp_mean(_lib.c_void_p(big.ctypes.data), _lib.c_void_p(z.ctypes.data), _lib.c_void_p(z.ctypes.data),
                                _lib.c_void_p(ones.ctypes.data), _lib.c_int(65536), _lib.c_int(1), _lib.c_long(65536),
                                _lib.c_void_p(ts.data_ptr()), _lib.c_void_p(val.data_ptr()), _lib.c_void_p(out.data_ptr()),
                                _lib.c_void_p(out.data_ptr()), _lib.c_void_p(0))
    torch.cuda.synchronize()
    assert rc == -1 and bool((out == 777.0).all())


# ------------------------------------------------------------------------------------------------------------------ peak_scale
@pytest.mark.parametrize("nch", (1, 2))
@pytest.mark.parametrize("ns", (1, 63, 64, 65, 16640))
def test_peak_scale_against_numpy_f32(ns, nch):
    from sar_ssl_amd import hip, parity
    rs = np.random.RandomState(ns * 3 + nch)
    x = (0.2 * rs.standard_normal((4, ns, nch))).astype(np.float32)
    x[0, -1, -1] = np.float32(-1.75)                                                             # the peak in the last sample of the last channel
    x[1] = 0.0                                                                                   # a zero item stays zero
    x[3, 0, 0] = np.float32(3.5)                                                                 # ... and in the first
    xd = torch.from_numpy(x.copy()).cuda()
    pk = torch.full((4,), float("nan"), device="cuda")
    got_pk = hip.peak_scale(xd, pk)
    torch.cuda.synchronize()
    assert got_pk.data_ptr() == pk.data_ptr()
    peak = np.abs(x).reshape(4, -1).max(axis=1)
    assert peak.dtype == np.float32 and np.array_equal(pk.cpu().numpy(), peak) and peak[0] == 1.75 and peak[1] == 0 and peak[3] == 3.5
    want = x * (np.float32(0.9) / (peak + np.float32(1e-8)))[:, None, None]
    assert want.dtype == np.float32
    got = xd.cpu().numpy()
    assert not got[1].any()
    g = parity.LOCATADS["peak_scale"]
    d = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max() / 0.9)
    print("PARITY peak_scale[ns=%d,nch=%d] measured=%.3e of the peak, tol=%.3e" % (ns, nch, d, min(g["gate"], g["cap"])))
    assert d <= min(g["gate"], g["cap"])


def test_peak_scale_reports_what_is_not_finite():
    from sar_ssl_amd import hip
    x = torch.full((3, 65, 2), 0.25, device="cuda")
    x[0, 64, 1] = float("nan")
    x[2, 3, 0] = float("-inf")
    pk = hip.peak_scale(x).cpu().numpy()
    assert np.isnan(pk[0]) and pk[1] == 0.25 and np.isnan(pk[2])
    assert bool(torch.isnan(x[0]).all()) and bool(torch.isnan(x[2]).all()) and bool((x[1] == 0.25 * (np.float32(0.9) / (np.float32(0.25) + np.float32(1e-8)))).all())


# ------------------------------------------------------------------------------------------------------------------ the generator
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return cases.build_tree(str(tmp_path_factory.mktemp("locata_ds_gpu")))


def test_generate_writes_the_restated_items_and_repeats_byte_for_byte(tree, tmp_path):
    from sar_ssl_amd import locatads, parity
    from sar_ssl_amd.dataset import read_wav_pcm16
    g = parity.LOCATADS["generate"]
    worst_pcm, worst_label = 0.0, 0.0
    for stage in cases.STAGES:
        corpus = locatads.TdoaCorpus(tree, stage, sort=True)
        plans, labels = locatads.generate(tree, str(tmp_path / "a"), stage, data_num=8, batch=3, sort=True, corpus=corpus)   # 3 + 3 + 2
        assert len(plans) == 8 and labels.dtype == np.float32
        rs = np.random.RandomState(locatads.SEEDS[stage])
        for i, p in enumerate(plans):
            assert p == corpus.plan(rs)                                                          # the reference's draws, in sequence
            x, tdoa = corpus.restate_item(p)
            pcm, fs = read_wav_pcm16(str(tmp_path / "a" / stage / ("%d.wav" % i)))
            assert fs == 16000 and pcm.shape == (cases.NS, 2)
            worst_pcm = max(worst_pcm, float(np.abs(pcm.astype(np.float64) - x * 32767.0).max()))
            info = np.load(str(tmp_path / "a" / stage / ("%d_info.npz" % i)))
            assert info.files == ["TDOA"] and info["TDOA"].dtype == np.float32 and info["TDOA"].shape == () and info["TDOA"] == labels[i]
            worst_label = max(worst_label, abs(float(labels[i]) - float(np.float32(tdoa))) / abs(float(np.float32(tdoa))))
        assert sorted(os.listdir(str(tmp_path / "a" / stage))) == sorted(["%d.wav" % i for i in range(8)] + ["%d_info.npz" % i for i in range(8)])
        locatads.generate(tree, str(tmp_path / "b"), stage, data_num=8, batch=3, sort=True, corpus=corpus)
        for f in os.listdir(str(tmp_path / "a" / stage)):
            assert open(str(tmp_path / "a" / stage / f), "rb").read() == open(str(tmp_path / "b" / stage / f), "rb").read(), f
        with pytest.raises(FileExistsError):
            locatads.generate(tree, str(tmp_path / "b"), stage, data_num=8, batch=3, sort=True, corpus=corpus)
    check("locatads.generate pcm (PCM-16 steps)", worst_pcm, g["pcm_steps"])
    print("PARITY locatads.generate label measured=%.3e tol=%.3e" % (worst_label, g["label"]))
    assert worst_label <= g["label"]


# ------------------------------------------------------------------------------------------------------------------ the sweep
def _model(mode):
    """A downstream model at TDOA's shape (64 frames) with seeded weights, dropout at its default, and its flat buffers."""
    from sar_ssl_amd import model, runtime
    dev = torch.device("cuda:0")
    torch.manual_seed(11)
    net = model.SARSSL(sig_shape=(256, 64, 2, 2), pretrain=False, device=dev, downstream_token="all", downstream_head="mlp",
                       downstream_embed="spat", downstream_dlabel=1)
    net.to(dev)
    return (net.train() if mode else net.eval()), runtime.FlatParams(net)


def test_one_training_step_and_one_evaluation_batch_of_the_sweep(tree, tmp_path):
    """run_downstream's LOCATA branch on a generated corpus: a training batch (LOCATA mixed 1 : 1 with simulated segments) and a
    validation batch (LOCATA only) from its loaders, through graph.DownstreamStepGraph in hybrid mode - finite, and the replayed step
    equal to the launch-by-launch step bit for bit (loss words and parameters), as tests/test_gpu_downstream_graph.py asserts for the
    simulated sweep."""
    import types
    from sar_ssl_amd import dataset, locatads, run_downstream as rd, runtime
    from sar_ssl_amd.graph import DownstreamStepGraph
    real, sim = str(tmp_path / "real_ds_locata"), str(tmp_path / "simu_ds" / "train")
    for stage in ("train", "val"):
        locatads.generate(tree, real, stage, data_num=6, batch=4, sort=True)
    cases.write_simulated(os.path.join(sim, "R1"), 3)
    args = types.SimpleNamespace(ds_specifics={"real_sim_ratio": [1, 1]})
    dirs = {"micsig_real": real, "micsig_train_simu": sim}
    data = rd.LocataData(args, dirs, 16000, dataset.Selecting(select_range=[0, cases.NS]), torch.device("cuda:0"))
    assert data.new_task() == 1
    batches = {}
    for stage, seed in (("train", 5), ("val", 6), ("test_large", 7)):
        if stage == "test_large":                                                                # reads <corpus>/test: not generated here
            with pytest.raises(ValueError, match="no segments"):
                data.loader(0, stage, 4, 4)
            continue
        loader = data.loader(0, stage, 8, 4)
        assert len(loader) == 2 and len(loader.dataset_list) == (2 if stage == "train" else 1)
        np.random.seed(seed)
        sig, lab = next(iter(loader))
        assert sig.shape == (4, cases.NS, 2) and sig.dtype == torch.float32 and sig.is_cuda and bool(torch.isfinite(lab["TDOA"]).all())
        batches[stage] = (sig.contiguous(), (lab["TDOA"][:, None] * 16000).contiguous())         # STFTLearner.get_tar_batch
        if stage == "val":
            assert bool(torch.isnan(lab["T60"]).all())                                          # LOCATA only
    runtime.set_precision("hybrid")
    try:
        res = {}
        for form in ("captured", "eager"):
            net, flat = _model(True)
            g = DownstreamStepGraph(net, flat, lr=1e-3)
            sig, tar = batches["train"]
            loss = (g.step if form == "captured" else g.step_eager)(pcm=sig, target=tar).clone()
            net.eval()
            sig, tar = batches["val"]
            ev = (g.eval_step if form == "captured" else g.eval_step_eager)(pcm=sig, target=tar).clone()
            torch.cuda.synchronize()
            res[form] = (loss.cpu(), ev.cpu(), flat.flat.clone())
            assert g.skipped_steps() == 0
        for k in range(2):
            assert bool(torch.isfinite(res["captured"][k]).all()), res["captured"][k]
            assert torch.equal(res["captured"][k], res["eager"][k]), (k, res["captured"][k], res["eager"][k])
        assert torch.equal(res["captured"][2], res["eager"][2])
    finally:
        runtime.set_precision("bf16")
