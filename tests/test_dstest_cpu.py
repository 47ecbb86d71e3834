"""Downstream test stage (``run_downstream.py --ds-test``), the parts that need no GPU: the no-information baseline against the reference's
numbers (fixture F19, ``wo_info.*``), the command line and the run directory the stage derives from it, the learning-rate index rule and
the t-SNE helper."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import GOLD, ROOT


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_dstest", os.path.join(ROOT, "tools", "make_golden_dstest.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _f19():
    return np.load(os.path.join(GOLD, "f19_dstest.npz"), allow_pickle=False)


@pytest.mark.parametrize("task", ["TDOA", "T60"])
def test_mae_wotrain_on_a_cpu_learner_vs_reference(task):
    """40 training labels, 37 test labels, batches of 16: the seven numbers of the reference's mae_wotrain.  Relative 1e-5 covers the f32
    summation order over 40 values (the reference sums the same f32 values; 40 * 2^-24 = 2.4e-6)."""
    from sar_ssl_amd import learner, model
    gen = _generator()
    c = gen.TDOA if task == "TDOA" else gen.T60
    net = model.SARSSL(sig_shape=(256, 8, 2, 2), pretrain=False, device="cpu", downstream_token="all", downstream_head="mlp",
                       downstream_embed=c["embed"], downstream_dlabel=1)
    lrn = learner.STFTLearner(net, win_len=512, win_shift_ratio=0.5, nfft=512, fre_used_ratio=1, fs=16000, task=task, ch_mode="M")
    assert lrn.device == "cpu" and lrn._flat is None
    got = lrn.mae_wotrain(gen.label_loader(c, train=True), gen.label_loader(c))
    ref = _f19()["wo_info." + task]
    assert len(got) == 7 and all(isinstance(v, float) for v in got)
    for name, g, r in zip(gen.WO_INFO_NAMES, got, ref):
        print("wo_info", task, name, g, r)
        assert abs(g - r) <= 1e-5 * abs(r), (name, g, r)
    if task == "TDOA":                                                       # targets are in samples: get_tar_batch's x 16000
        lab = gen.labels(c).numpy()
        assert abs(got[1] - float(lab.min()) * 16000) <= 1e-5 * abs(got[1])


def _parse(mode, extra=()):
    from sar_ssl_amd.opt import opt_downstream
    opts = opt_downstream()
    args = opts.parse(["--ds-test", "--simu-exp", "--test-mode", mode, "--ds-trainmode", "finetune", "--ds-task", "TDOA", "--ds-nsimroom", "32",
                       "--ds-num", "8", "--ds-bs-set", "4", "--ds-eval-num", "4", "--work-dir", "/w", "--time", "t1", "--gpu-id", "0,"] + list(extra))
    return args, opts.dir()


@pytest.mark.parametrize("mode", ["cal_metric", "cal_metric_wo_info", "vis_embed"])
def test_command_line_and_run_directory(mode):
    from sar_ssl_amd import run_downstream as rd
    args, dirs = _parse(mode, ["--ds-lr-set", "0.0001"])
    assert args.ds_test and not args.ds_train and args.test_mode == mode and args.simu_exp
    st = args.ds_setting["TDOA"]
    lr = st["lr_set"][rd.ds_test_lr_index(st["lr_set"])]
    d = rd.run_dir(dirs, args.ds_trainmode, "TDOA", st["num"], lr, st["bs_set"][0], 0)
    assert d == "/w/SAR-SSL/exp/TDOA/t1/finetune-all-mlp-8-0.0001-4-0-spat-sim_R32"
    assert rd.run_dir(dirs, "lineareval", "T60", 800, 0.0005, 8, 3) == "/w/SAR-SSL/exp/T60/t1/lineareval-all-mlp-800-0.0005-8-3-spat-sim_R32"
    want = {"train": 8, "test": 4} if mode != "vis_embed" else {"train": 8000, "test": 4}
    assert rd.ds_test_data_num(mode, st["num"], args.ds_eval_num) == want
    assert rd.ds_test_data_num(mode, 800) == ({"train": 800, "test": 4000} if mode != "vis_embed" else {"train": 8000, "test": 8000})
    assert rd.TEST_BS == 16


def test_lr_index_rule():
    """The reference reads lr_set[1]; a one-entry build-side --ds-lr-set leaves index 0."""
    from sar_ssl_amd import run_downstream as rd
    assert rd.ds_test_lr_index([0.001, 0.0005]) == 1
    assert rd.ds_test_lr_index([0.0001]) == 0
    args, _ = _parse("cal_metric")                                           # the reference's four-entry sweep
    lr_set = args.ds_setting["TDOA"]["lr_set"]
    assert lr_set[rd.ds_test_lr_index(lr_set)] == 0.0005


def test_vis_tsne_small_sets():
    pytest.importorskip("sklearn")
    pytest.importorskip("matplotlib")
    from sar_ssl_amd.common.utils import vis_TSNE
    rng = np.random.default_rng(0)
    data, label = rng.standard_normal((12, 16)).astype(np.float32), rng.uniform(-8, 8, (12, 1)).astype(np.float32)
    plt, out = vis_TSNE(data=data, label=label)
    plt.close()
    assert out["data"].shape == (12, 2) and np.isfinite(out["data"]).all()
    assert out["label"] is label
