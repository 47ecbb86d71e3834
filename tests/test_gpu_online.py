"""GPU: online simulated pretraining (onlinesig.OnlineSignalLoader, run_pretrain.py --simu-online) - every item against the f64
restatement roomsim.restate_sig of its restated configuration and plan (parity.SIMSIG), the items as functions of their global index,
and the command end to end in a child process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import online_cases as oc
import simsig_cases as sc
from conftest import ROOT, check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T_SMALL, NS_SMALL, B, DATASET_SZ, CHUNK = 0.272, 4352, 4, 12, 8


@pytest.fixture(scope="module")
def bank(tmp_path_factory):
    from sar_ssl_amd import rirsynth
    top, _ = oc.write_tree(tmp_path_factory.mktemp("spk"), single=2000)
    return rirsynth.DeviceSourceBank(top, oc.FS, DEV, sort=True)


def _loader(bank, batch=B, dataset_sz=DATASET_SZ, **kw):
    from sar_ssl_amd import onlinesig
    return onlinesig.OnlineSignalLoader(bank, dataset_sz, batch, T_SMALL, 1, DEV, chunk=CHUNK, log=kw.pop("log", None), **dict(sc.SMALL, **kw))


def _epoch(ld, epoch=0):
    """One iteration -> ({g: (Ns, 2) int16 array}, the batches' shapes)."""
    ld.set_epoch(epoch)
    items, shapes = {}, []
    for step, (pcm,) in enumerate(ld):
        assert pcm.dtype == torch.int16 and pcm.is_cuda and pcm.shape[1:] == (NS_SMALL, 2)
        shapes.append(pcm.shape[0])
        host = pcm.cpu().numpy()
        for j, g in enumerate(ld.indices(epoch, step)):
            items[g] = host[j]
    return items, shapes


_RIRS = {}


def _restated(ld, g):
    """roomsim.restate_sig of item g: its restated configuration and plan, the accepted attempt's tail noise (rooms are restated once)."""
    from sar_ssl_amd import roomsim
    plan, room = ld.restate_plan(g), g // ld.reuse
    attempt = ld.attempts[room] - 1
    if (room, attempt) not in _RIRS:
        n_len = roomsim.plan_rir(plan["cfg"])["n_len"]
        _RIRS[room, attempt] = (roomsim.restate_cfg(plan["cfg"], roomsim.numpy_noise(ld.seed, room, attempt, 2, n_len)),
                                roomsim.restate_cfg(plan["cfg"], None, dp=True))
    rir, dp = _RIRS[room, attempt]
    return roomsim.restate_sig(plan, rir=rir, rir_dp=dp)


@pytest.mark.parametrize("reuse", [1, 2])
def test_online_items_against_the_restatement(bank, reuse):
    from sar_ssl_amd import parity
    ld = _loader(bank, noise="numpy", reuse=reuse)
    items, shapes = _epoch(ld)
    assert shapes == [4, 4, 4] and sorted(items) == list(range(12)) and sorted(ld.attempts) == list(range(12 // reuse))
    worst = 0.0
    for g in range(12):
        want = _restated(ld, g)
        d = np.abs(items[g].astype(np.int32) - want.astype(np.int32))
        share = float((d != 0).mean())
        print("PARITY online.reuse%d.g%d max_step measured=%d tol=%d share=%.4f" % (reuse, g, d.max(), parity.SIMSIG["pcm_step"], share))
        assert d.max() <= parity.SIMSIG["pcm_step"], (g, int(d.max()))
        assert share < parity.SIMSIG["share_bound"], (g, share)
        assert np.abs(items[g]).max() >= 29000                  # the peak of mic / direct path sits at 0.9 of full scale
        worst = max(worst, share)
    check("online.reuse%d.share" % reuse, worst, parity.SIMSIG["share_bound"])
    if reuse == 2:
        assert all(not np.array_equal(items[2 * k], items[2 * k + 1]) for k in range(6))


@pytest.fixture(scope="module")
def device_runs(bank):
    ld = _loader(bank)
    first, shapes = _epoch(ld)
    return ld, first, shapes


def test_online_epochs_are_reproducible_and_differ(bank, device_runs):
    ld, first, shapes = device_runs
    assert shapes == [4, 4, 4] and len(ld) == 3 and sorted(first) == list(range(12))
    again, _ = _epoch(ld)
    assert all(first[g].tobytes() == again[g].tobytes() for g in first)
    second, _ = _epoch(ld, 1)
    assert sorted(second) == list(range(12, 24)) and all(not np.array_equal(first[g], second[g + 12]) for g in first)
    assert all(29000 <= np.abs(x).max() <= 32767 for x in second.values())


def test_online_items_do_not_depend_on_the_batch_size(bank, device_runs):
    _, first, _ = device_runs
    six, shapes = _epoch(_loader(bank, batch=6))
    assert shapes == [6, 6] and all(first[g].tobytes() == six[g].tobytes() for g in first)


def test_online_last_batch_is_ragged_where_the_epoch_says_so(bank, device_runs):
    _, first, _ = device_runs
    ten, shapes = _epoch(_loader(bank, dataset_sz=10, reuse=2))
    assert shapes == [4, 4, 2] and sorted(ten) == list(range(10))
    assert ten[0].tobytes() == first[0].tobytes()               # item 0 lies in room 0 with either reuse
    assert all(not np.array_equal(ten[2 * k], ten[2 * k + 1]) for k in range(5))


def test_online_skipped_item_is_replaced_and_logged(bank, monkeypatch):
    from sar_ssl_amd import roomsim
    judge = roomsim.judge_on_device

    def never(rir, n_len, rir_dp, dp_len, T60_specify, ids=None, attempt=0, fs=oc.FS):
        lab = judge(rir, n_len, rir_dp, dp_len, T60_specify, ids, attempt, fs)
        if 1 in ids:
            lab["flags"][list(ids).index(1)] = 1
        return lab

    monkeypatch.setattr(roomsim, "judge_on_device", never)
    monkeypatch.setattr(roomsim, "MAX_ATTEMPTS", 2)
    lines = []
    items, shapes = _epoch(_loader(bank, dataset_sz=4, log=lines.append))
    assert shapes == [4] and items[1].tobytes() == items[2].tobytes() and items[0].tobytes() != items[2].tobytes()
    assert any("item 1 " in ln and "skipped" in ln for ln in lines) and any("item 1 is replaced by item 2" in ln for ln in lines)


def test_run_pretrain_simu_online_entry_point(tmp_path):
    """`run_pretrain.py --pretrain --simu-exp --simu-online` in a child process: two epochs of two rendered batches each over a synthetic
    speaker tree, validation on a preval corpus the generator wrote; scalars with finite losses and no pretrain corpus on disk."""
    from sar_ssl_amd import roomsim
    work = tmp_path / "work"
    oc.write_tree(work / "data" / "SrcSig" / "wsj0", single=40000, sub="tr", scale=16)
    oc.write_tree(tmp_path / "valsrc", single=40000, sub="dt", scale=16)
    simu = work / "SAR-SSL" / "data" / "MicSig" / "simu"
    res = roomsim.simulate_signals(str(simu), "preval", 8, str(tmp_path / "valsrc"), device=DEV, batch=8, T=4.112, sort_sources=True, **sc.SMALL)
    assert res["written"] == list(range(8))
    cmd = [sys.executable, os.path.join(ROOT, "run_pretrain.py"), "--pretrain", "--simu-exp", "--simu-online", "--data-num", "8", "8",
           "--bs", "4", "4", "4", "--nepoch", "2", "--gpu-id", "0,", "--work-dir", str(work), "--workers", "2", "--time", "t0"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    recs = [json.loads(ln) for ln in open(work / "SAR-SSL" / "exp" / "pretrain" / "t0" / "scalars.jsonl").read().strip().splitlines()]
    assert len(recs) == 2 and [rec["epoch"] for rec in recs] == [1, 2]
    assert all(np.isfinite(rec["loss_train"]) and np.isfinite(rec["loss_val"]) and rec["loss_train"] > 0 for rec in recs)
    assert not (simu / "pretrain").exists() and sorted(os.listdir(simu)) == ["preval"]
