"""CPU: the real-data downstream branch's host side (sar_ssl_amd/rirsynth.py, opt.py) against fixture F20 of the real reference
(tools/make_golden_rirmix.py): the f64 numpy / scipy restatement of an item reproduces every stored output, the host plan reproduces
every stored draw, the options are the reference's, cross_validation_datadir is the reference's."""
import functools
import importlib.util
import os
import random

import numpy as np
import pytest

from conftest import GOLD, ROOT, check

CAP = 1.5e-5                      # half a PCM-16 step: the hard cap on any distance between peak-normalised renderings


@functools.lru_cache(maxsize=None)
def _gen():
    spec = importlib.util.spec_from_file_location("make_golden_rirmix", os.path.join(ROOT, "tools", "make_golden_rirmix.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def _f20():
    return dict(np.load(os.path.join(GOLD, "f20_rirmix.npz"), allow_pickle=False))


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """The fixture's tree on disk and the three banks over it (sorted listings, as the fixture was made)."""
    import __graft_entry__ as g
    from sar_ssl_amd import _lib, rirsynth
    if not os.path.exists(_lib.LIB_PATH):
        g.build()                                             # the noise recordings are probed and read by the library's PCM reader
    gen, f = _gen(), _f20()
    root = gen.restore_tree(str(tmp_path_factory.mktemp("f20_tree")), f)
    d = gen.dirs_of(root)
    measured = rirsynth.MeasuredBank(d["real_rooms"], fs=gen.FS, sort=True)
    simulated = rirsynth.SimulatedBank([d["rir_train_simu"]], fs=gen.FS, c=gen.C, sort=True)
    sources = rirsynth.SourceBank(d["src"], fs=gen.FS, sort=True)
    return dict(root=root, dirs=d, measured=measured, simulated=simulated, sources=sources)


def _rel(tree, path):
    return "" if path is None else os.path.relpath(str(path), tree["root"])


def _plans(tree):
    """{fixture prefix: plan} of every stored item, planned as the reference drew it."""
    from sar_ssl_amd import rirsynth
    gen = _gen()
    kw = dict(T=gen.T, fs=gen.FS, snr_range=gen.SNR_RANGE)
    plans = {}
    f = _f20()
    for j in range(gen.ITEMS):
        i, k = int(f["measured_ids"][j]), int(f["simulated_ids"][j])
        plans["measured/%d/" % j] = rirsynth.plan_measured(np.random.RandomState(0), i, gen.SEED, tree["measured"], tree["sources"], **kw)
        plans["simulated/%d/" % j] = rirsynth.plan_simulated(np.random.RandomState(0), k, gen.SEED, tree["simulated"], tree["sources"], nmic=gen.NMIC, **kw)
    rs = np.random.RandomState(gen.OUTER_SEED)
    for i in range(gen.OUTER_ITEMS):
        plans["outer/%d/" % i] = rirsynth.plan_random(rs, ["measured", "simulated"], gen.SEED, tree["measured"], tree["simulated"], tree["sources"],
                                                      nmic=gen.NMIC, **kw)
    return plans


def test_banks_list_the_tree_as_the_reference_did(tree):
    f = _f20()
    assert [_rel(tree, p) for p in tree["measured"].files] == [str(x) for x in f["rir_files_measured"]]
    assert [_rel(tree, p) for p in tree["simulated"].files] == [str(x) for x in f["rir_files_simulated"]]
    assert tree["sources"].spk_ids == [str(x) for x in f["speakers"]]
    assert sorted(len(n) for n in tree["measured"].noise_files) == [0, 0, 0, 0, 0, 2]       # one RIR of one room has two noise recordings


def test_plan_reproduces_every_draw(tree):
    f, gen = _f20(), _gen()
    plans = _plans(tree)
    assert len(plans) == 2 * gen.ITEMS + gen.OUTER_ITEMS
    for pre, p in plans.items():
        assert (p["variant"] == "simulated") == bool(f[pre + "simulated"]), pre
        assert _rel(tree, p["rir_file"]) == str(f[pre + "rir_file"]), pre
        assert _rel(tree, p["noise_file"]) == str(f[pre + "noise_file"]) and p["noise_start"] == int(f[pre + "noise_start"]), pre
        assert p["utt_idx"] == int(f[pre + "utt_idx"]) and p["crop_start"] == int(f[pre + "crop_start"]), pre
        assert [_rel(tree, u) for u in p["utt_files"]] == [str(x) for x in f[pre + "utt_files"]], pre
        assert p["snr"] == float(f[pre + "snr"]), pre
        for k in ("T60", "DRR", "C50", "ABS"):
            assert p["labels"][k].dtype == np.float32 and np.array_equal(p["labels"][k], f[pre + "label_" + k]), (pre, k)
        if p["variant"] == "simulated":
            w = p["white"]
            assert np.array_equal(w[:gen.WHITE_HEAD], f[pre + "white_head"]), pre
            assert np.array_equal(np.array([w.sum(), (w ** 2).sum()]), f[pre + "white_sums"]), pre
    assert {bool(str(f["measured/%d/noise_file" % i])) for i in range(gen.ITEMS)} == {True, False}   # measured items with and without recorded noise
    assert len({str(f["simulated/%d/rir_file" % i]) for i in range(gen.ITEMS)}) == 2
    assert {bool(f["outer/%d/simulated" % i]) for i in range(gen.OUTER_ITEMS)} == {True, False}     # the outer stream serves both variants


def test_f64_restatement_reproduces_every_output(tree):
    """The reference forms the item in mixed f32 / f64 (f32 RIRs and noise recordings, f64 sources) and F20 stores it as f32, so the distance
    is not zero: printed per item, gated at the hard cap."""
    from sar_ssl_amd import rirsynth
    f, gen = _f20(), _gen()
    worst = {"measured": 0.0, "simulated": 0.0}
    for pre, p in _plans(tree).items():
        out = rirsynth.restate_item(p, tree["measured"], tree["simulated"], fs=gen.FS, c=gen.C)
        assert out.shape == (gen.NS, gen.NMIC) and out.dtype == np.float64
        d = float(np.abs(out - f[pre + "out"]).max())
        print("restatement vs reference %s %s: %.3e" % (pre, p["variant"], d))
        worst[p["variant"]] = max(worst[p["variant"]], d)
    for v, d in worst.items():
        check("f64 restatement vs F20, " + v, d, CAP)


def test_restated_diffuse_field_is_the_references_two_scipy_calls():
    """restate_diffuse pads by hand (so that Ns < 256 is defined); from Ns = 256 on it is scipy.signal.stft / istft as the reference calls them."""
    import scipy.signal
    from sar_ssl_amd import rirsynth
    rs = np.random.RandomState(1)
    white = rs.standard_normal((4352, 2))
    C = rirsynth.mixing_table(np.array([[0, 0, 0], [0.08, 0, 0.0]]))
    _, _, N = scipy.signal.stft(white.T, window="hann", nperseg=256, noverlap=0.75 * 256, nfft=256)
    X = np.einsum("fmn,mft->nft", np.conj(C), N)
    _, y = scipy.signal.istft(X, window="hann", nperseg=256, noverlap=0.75 * 256, nfft=256)
    y = y.T
    assert np.array_equal(rirsynth.restate_diffuse(white, C), y / (np.max(y) + 1e-8))
    assert rirsynth.restate_diffuse(white[:64], C).shape == (64, 2)
    with pytest.raises(AssertionError):
        rirsynth.restate_diffuse(white[:100], C)


def test_banks_refuse_what_the_renderer_does_not_do(tree, tmp_path):
    from sar_ssl_amd import rirsynth
    gen, f = _gen(), _f20()
    for name, bad in (("fs", {"fs": np.array(48000)}), ("npoint", None), ("nsrc", None)):
        root = gen.restore_tree(str(tmp_path / name), f)
        stem = os.path.join(root, "real/ACE/Office_1/conf0/rir_mic0")
        if bad is not None:
            np.savez(stem + "_info.npz", **dict(dict(np.load(stem + "_info.npz")), **bad))
        else:
            h = np.load(stem + ".npy")
            np.save(stem + ".npy", np.concatenate([h, h], axis=0 if name == "npoint" else 3))
        with pytest.raises(ValueError, match={"fs": "not resampled", "npoint": "npoint = 2", "nsrc": "nsrc = 2"}[name]):
            rirsynth.MeasuredBank(gen.dirs_of(root)["real_rooms"], fs=gen.FS)


def test_cross_validation_datadir_is_the_references(tree):
    from sar_ssl_amd.common.utils import cross_validation_datadir
    f = _f20()
    random.seed(int(f["cv_seed"]))
    cv = cross_validation_datadir(tree["dirs"]["rir_real"], sort=True)
    assert len(cv) == 3
    for t, trial in enumerate(cv):
        for k in ("train", "val", "test"):
            assert [_rel(tree, p) for p in trial[k]] == [str(x) for x in f["cv/%d/%s" % (t, k)]], (t, k)


REAL = ["--ds-train", "--ds-trainmode", "finetune", "--time", "T0", "--work-dir", "/w"]


def test_opt_downstream_real_data_settings():
    from sar_ssl_amd.opt import opt_downstream
    o = opt_downstream()
    a = o.parse(REAL + ["--ds-task", "T60"])
    assert a.ds_specifics == {"task": ["T60"], "data": "real_ace", "real_sim_ratio": [1, 1]}
    for t in ("DRR", "C50", "T60", "ABS"):
        assert a.ds_setting[t] == {"nepoch": 200, "num": 3200, "lr_set": [0.001, 0.0001], "bs_set": [16], "ntrial": 1}
    assert a.ds_setting["TDOA"]["num"] == 80000
    d = o.dir()
    assert d["rir_real"] == "/w/SAR-SSL/data/RIR/real/ACE" and d["rir_train_simu"] == "/w/SAR-SSL/data/RIR/simu/train"
    assert (d["srcsig_train"], d["srcsig_val"], d["srcsig_test"]) == tuple("/w/data/SrcSig/wsj0/" + s for s in ("tr", "dt", "et"))
    assert d["log_task_finetune"] == "/w/SAR-SSL/exp/TASK/T0/finetune-all-mlp-NUM-LR-BAS-TRI-spat-real_train1real1sim_valreal"
    assert "micsig_val_simu" not in d
    nums = {("finetune", (1, 0)): 1600, ("finetune", (0, 1)): 32000, ("scratchLOW", (1, 0)): 1600, ("scratchLOW", (1, 1)): 16000,
            ("scratchLOW", (0, 1)): 32000}
    for (mode, ratio), num in nums.items():
        a = opt_downstream().parse(["--ds-train", "--ds-trainmode", mode, "--ds-task", "C50", "--ds-real-sim-ratio", str(ratio[0]), str(ratio[1])])
        assert a.ds_setting["C50"]["num"] == num, (mode, ratio)
    with pytest.raises(Exception, match="Undefined trainmode"):
        opt_downstream().parse(["--ds-train", "--ds-trainmode", "lineareval", "--ds-task", "C50"])
    a = opt_downstream().parse(REAL + ["--ds-task", "ABS", "--ds-nepoch", "1", "--ds-num", "16", "--ds-lr-set", "0.01", "--ds-bs-set", "8", "--ds-eval-num", "16"])
    assert a.ds_setting["ABS"] == {"nepoch": 1, "num": 16, "lr_set": [0.01], "bs_set": [8], "ntrial": 1} and a.ds_eval_num == 16


def test_opt_downstream_still_refuses_what_is_out_of_scope(capsys):
    from sar_ssl_amd.opt import opt_downstream
    with pytest.raises(SystemExit) as e:
        opt_downstream().parse(REAL + ["--ds-task", "TDOA"])
    assert "LOCATA" in str(e.value) and "RandomMicSigDataset" in str(e.value)
    with pytest.raises(SystemExit) as e:
        opt_downstream().parse(["--ds-test", "--ds-task", "T60"])
    assert "--ds-test" in str(e.value) and "simulated" in str(e.value)
    a = opt_downstream().parse(["--ds-train", "--simu-exp", "--ds-task", "TDOA", "--ds-nsimroom", "8"])          # the simulated branch is untouched
    assert a.ds_setting["TDOA"]["bs_set"] == [8] and a.ds_specifics == {"task": ["TDOA"]}
