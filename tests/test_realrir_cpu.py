"""CPU: the host side of gen_real_rir.py - realrir.restate_resample against scipy.signal.resample_poly, dataset.read_wav over the four
sample formats, and realrir.gen_rir / gen_noise on the f64 restatement against fixture F25 (the reference's own ACERIRDataset over the
synthetic tree of tests/realrir_cases.py, tools/make_golden_realrir.py); the written tree as input of rirsynth.MeasuredBank and of the
leave-one-room-out splits; the command line's refusals."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sarssl_boot  # noqa: E402,F401
import realrir_cases as cases  # noqa: E402

F25 = os.path.join(ROOT, "tests", "golden", "f25_realrir_ace.npz")
LABELS = ("T60fromDataset", "DRRfromDataset", "DRR", "C50", "ABS")


@pytest.mark.parametrize("up,down,n", [(1, 3, 1000), (2, 3, 1001), (160, 441, 1000), (2, 1, 333), (3, 1, 100), (16000, 48000, 1000),
                                       (7, 7, 50), (1, 3, 1), (2, 3, 7)])
def test_restatement_equals_scipy(up, down, n):
    import scipy.signal
    from sar_ssl_amd import realrir
    x = np.random.RandomState(up * 1000 + down).standard_normal((n, 3))
    want = scipy.signal.resample_poly(x, up, down, axis=0)
    got = realrir.restate_resample(x, up, down)
    assert got.shape == want.shape and got.shape[0] == -(-n * up // down)
    assert np.abs(got - want).max() <= 1e-12
    assert np.array_equal(realrir.restate_resample(x[:, 0], up, down), got[:, 0])


@pytest.mark.parametrize("fmt,step", [("pcm16", 2.0 ** -15), ("pcm24", 2.0 ** -23), ("pcm32", 2.0 ** -31), ("float32", 0.0)])
@pytest.mark.parametrize("extensible", [False, True])
def test_read_wav_round_trips_the_sample_formats(tmp_path, fmt, step, extensible):
    from sar_ssl_amd.dataset import read_wav
    x = np.clip(np.random.RandomState(5).standard_normal((333, 3)) * 0.3, -0.99, 0.99)
    x[0] = (-1.0, 0.0, 0.5)
    p = str(tmp_path / "x.wav")
    back = cases.write_wav(p, x, 44100, fmt, extensible)
    got, fs = read_wav(p)
    assert fs == 44100 and got.dtype == np.float64 and got.shape == x.shape
    assert np.array_equal(got, back) and np.abs(got - x).max() <= max(step / 2, 2.0 ** -25)
    if fmt == "pcm16":
        raw, _ = read_wav(p, raw_pcm16=True)
        assert raw.dtype == np.int16 and np.array_equal(raw.astype(np.float64) / 32768.0, got)


def test_read_wav_refuses_other_formats_by_name(tmp_path):
    import struct
    from sar_ssl_amd.dataset import read_wav
    for tag, bits, word in ((7, 8, "mu-law"), (6, 8, "A-law"), (1, 8, "PCM, 8 bits"), (3, 64, "IEEE float, 64 bits")):
        body = b"\x00" * 64
        fmt = struct.pack("<HHIIHH", tag, 1, 8000, 8000 * bits // 8, bits // 8, bits)
        chunks = b"WAVE" + b"fmt " + struct.pack("<I", 16) + fmt + b"data" + struct.pack("<I", len(body)) + body
        p = str(tmp_path / ("t%d_%d.wav" % (tag, bits)))
        with open(p, "wb") as f:
            f.write(b"RIFF" + struct.pack("<I", len(chunks)) + chunks)
        with pytest.raises(ValueError, match=word):
            read_wav(p)
    chunks = b"WAVE" + b"fmt " + struct.pack("<I", 8) + b"\x01\x00\x01\x00\x40\x1f\x00\x00" + b"data" + struct.pack("<I", 4) + b"\x00" * 4
    p = str(tmp_path / "short_fmt.wav")
    with open(p, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(chunks)) + chunks)
    with pytest.raises(ValueError, match="short_fmt.wav: fmt chunk of 8 bytes"):
        read_wav(p)


@pytest.fixture(scope="module")
def written(tmp_path_factory):
    """The synthetic tree and what realrir writes for it on the f64 restatement -> (F25, save_dir, rir paths, noise paths)."""
    from sar_ssl_amd import realrir
    root = str(tmp_path_factory.mktemp("f25"))
    cases.build_tree(os.path.join(root, "in"))
    save = os.path.join(root, "real")
    rs = realrir.HostResampler()
    rir = realrir.gen_rir(os.path.join(root, "in", "ACE"), os.path.join(save, "ACE"), rs)
    noise = realrir.gen_noise(os.path.join(root, "in", "ACE"), os.path.join(save, "ACE_noise"), rs)
    return np.load(F25), save, rir, noise


def test_geometry_is_the_references():
    from sar_ssl_amd import realrir
    fx = np.load(F25)
    assert tuple(cases.ROOMS) == realrir.ROOMS and tuple(cases.ARRAYS) == realrir.ARRAYS
    for a in realrir.ARRAYS:
        assert np.array_equal(realrir.MIC_POS[a], fx["mic_pos/" + a]), a
    for r in realrir.ROOMS:
        assert np.array_equal(np.array(realrir.ROOM_SZ[r], np.float64), fx["room_sz/" + r]), r
    assert np.array_equal(realrir.MIC_POS["EM32"][7], realrir.MIC_POS["EM32"][5])              # (sic)
    assert [5, 7] not in realrir.selected_pairs("EM32") and [0, 1] not in realrir.selected_pairs("EM32") and len(realrir.selected_pairs("Lin8Ch")) == 18


def test_pairs_files_keys_and_labels_equal_f25(written):
    from sar_ssl_amd import realrir
    fx, save, rir, noise = written
    stems = [os.path.relpath(p, os.path.join(save, "ACE"))[:-4] for p in rir]
    assert stems == [str(s) for s in fx["pairs"]]                                             # the reference's pairs, in its order
    assert cases.tree_listing(os.path.join(save, "ACE")) == sorted([s + ".npy" for s in stems] + [s + "_info.npz" for s in stems])
    assert cases.tree_listing(os.path.join(save, "ACE_noise")) == [str(s) for s in fx["noise_files"]]
    assert sorted(os.path.relpath(p, os.path.join(save, "ACE_noise")) for p in noise) == [str(s) for s in fx["noise_files"]]
    worst = 0.0
    for k, p in enumerate(rir):
        info = dict(np.load(p[:-4] + "_info.npz"))
        assert sorted(info) == [str(s) for s in fx["info_keys"]] == sorted(realrir.INFO_KEYS)
        room, array = stems[k].split("/")[:2]
        assert np.array_equal(info["mic_pos"], fx["mic_pos/" + array][fx["mic_idx"][k]]) and np.array_equal(info["room_sz"], fx["room_sz/" + room])
        assert int(info["fs"]) == int(fx["fs"])
        got = np.array([float(info[key]) for key in LABELS])
        worst = max(worst, np.abs(got / fx["labels"][k] - 1.0).max())
    print("labels vs F25: max relative difference %.3e" % worst)
    assert worst <= 1e-9


def test_stored_arrays_equal_f25(written):
    from sar_ssl_amd.dataset import read_wav_pcm16
    fx, save, _, _ = written
    for array, (i, j) in cases.STORED_PAIRS.items():
        r = np.load(os.path.join(save, "ACE", "Office_2", array, "SP1_MP2-%d-%d.npy" % (i, j)))
        assert r.dtype == np.float32 and r.shape == (1, 2, 1600, 1)
        assert np.abs(r.astype(np.float64) - fx["rir/" + array]).max() <= 1e-9 * np.abs(fx["rir/" + array]).max()
        for typ in cases.NOISE_TYPES:
            pcm, fs = read_wav_pcm16(os.path.join(save, "ACE_noise", "Office_2", array, "_MP2-%d-%d_%s.wav" % (i, j, typ)))
            assert fs == cases.FS and pcm.shape == (4000, 2)
            assert np.abs(pcm.astype(np.int32) - fx["noise/%s/%s" % (array, typ)]).max() <= 1
    assert [str(s) for s in fx["noise_zero"]] == ["Office_1/Mobile/_MP2-%d-%d_Fan.wav" % p for p in ((1, 2), (1, 3), (2, 3))]
    for rel in fx["noise_zero"]:
        pcm, fs = read_wav_pcm16(os.path.join(save, "ACE_noise", str(rel)))
        assert pcm.shape == tuple(fx["noise_zero_shape"]) == (5 * cases.FS, 2) and not pcm.any()


def test_direct_path_rule_and_its_refusal():
    from sar_ssl_amd import realrir
    h = np.zeros(100)
    h[[10, 20, 30]] = (0.4, 1.0, 0.9)
    assert realrir.find_direct_path(h) == 20
    h[10] = 0.5
    assert realrir.find_direct_path(h) == 10                                                  # half the maximum counts
    assert realrir.find_direct_path(np.zeros(100)) is None
    with pytest.raises(ValueError, match="some.wav.*channel 2.*direct-path"):
        realrir.channel_labels(np.stack([h, np.zeros(100)], axis=1), 16000, "some.wav")


def test_written_tree_loads_as_a_measured_bank(written):
    from sar_ssl_amd import rirsynth
    from sar_ssl_amd.common.utils import cross_validation_datadir
    fx, save, rir, _ = written
    trials = cross_validation_datadir(os.path.join(save, "ACE"), sort=True)
    assert len(trials) == 7 and [os.path.basename(t["test"][0]) for t in trials] == sorted(cases.ROOMS)
    assert all(len(t["train"]) == 5 and len(t["val"]) == 1 for t in trials)
    bank = rirsynth.MeasuredBank(os.path.join(save, "ACE", "Office_1", "Mobile"), fs=cases.FS, sort=True)
    assert bank.nch == 2 and len(bank) == 6
    stems = [str(s) for s in fx["pairs"]]
    for f, lab, noise in zip(bank.files, bank.labels, bank.noise_files):
        k = stems.index(os.path.relpath(str(f), os.path.join(save, "ACE"))[:-4])
        assert np.allclose([lab["T60"], lab["DRR"], lab["C50"], lab["ABS"]], fx["labels"][k][[0, 2, 3, 4]], rtol=1e-6)
        mp = os.path.basename(str(f)).split("_")[1][:-4]
        assert sorted(os.path.basename(str(n)) for n in noise) == ["_%s_%s.wav" % (mp, t) for t in cases.NOISE_TYPES]
    with pytest.raises(ValueError, match="not resampled"):                                     # unchanged: a foreign rate is refused
        rirsynth.MeasuredBank(os.path.join(save, "ACE", "Office_1", "Mobile"), fs=8000, sort=True)


@pytest.mark.parametrize("name", ["DCASE", "Mesh", "MIR", "dEchorate", "BUTReverb"])
def test_unbuilt_datasets_exit_with_the_message(name, capsys):
    from sar_ssl_amd import realrir
    with pytest.raises(SystemExit) as e:
        realrir.main(["--dataset", name, "--read_dir", "x", "--save_dir", "y"])
    assert e.value.code != 0
    assert "only ACE is built" in capsys.readouterr().err
