"""Frozen-encoder probe stage (``--pretrain-frozen-encoder``), the parts that need no GPU: the model's key set against the reference's
(fixture state_dict_manifest_frozen.json), the command line, the probe inputs restated in numpy against what the reference fed its
encoders (fixture F17, ``probe.*``), and - where the reference tree is present - F17's loss recomputed live."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLD, ROOT


def _manifest():
    return json.load(open(os.path.join(GOLD, "state_dict_manifest_frozen.json")))["frozen"]


def _f17():
    return np.load(os.path.join(GOLD, "f17_frozen_step.npz"), allow_pickle=False)


def probe_inputs_np(x, idx, ch):
    """The two encoder inputs of the frozen stage from x (B, mic, F, T, reim), the masked frames idx (B, nm) and the masked channel ch (B)
    -> (spec_in, spat_in), both (B, F, T, 4) with c = reim * 2 + mic: the spectral encoder sees the UNMASKED channel at the MASKED frames
    only, the spatial encoder both channels at the visible frames."""
    x = np.asarray(x, dtype=np.float32)
    B, nmic, F, T, _ = x.shape
    visible = np.ones((B, T), dtype=np.float32)
    for b in range(B):
        visible[b, np.asarray(idx[b], dtype=np.int64)] = 0.0
    keep_ch = np.ones((B, nmic), dtype=np.float32)
    keep_ch[np.arange(B), np.asarray(ch, dtype=np.int64).reshape(-1)] = 0.0
    v = x.transpose(0, 2, 3, 4, 1)                                            # (B, F, T, reim, mic)
    spec = v * (1.0 - visible)[:, None, :, None, None] * keep_ch[:, None, None, None, :]
    spat = v * visible[:, None, :, None, None]
    return spec.reshape(B, F, T, 4), spat.reshape(B, F, T, 4)


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_frozen", os.path.join(ROOT, "tools", "make_golden_frozen.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_frozen_model_keys_order_and_shapes_equal_the_reference():
    from sar_ssl_amd import model
    net = model.SARSSL(sig_shape=(256, 256, 2, 2), pretrain=False, pretrain_frozen_encoder=True, device="cpu")
    man = _manifest()
    sd = net.state_dict()
    assert list(sd.keys()) == list(man.keys())
    assert {k: list(v.shape) for k, v in sd.items()} == man
    assert hasattr(net, "patch_mask") and not hasattr(net, "decoder") and not hasattr(net, "mlp_head") and not hasattr(net, "joint_head")
    assert net.spec_spat_decoder.proj[0].in_features == 768 and net.spec_decoder.proj[0].in_features == 512
    assert net.spat_decoder.proj[0].in_features == 512                           # (sic, code/model.py:481)
    # the three decoders reach the flat buffers as the 'decoder' group, behind the encoders' groups
    groups = dict(net.flat_param_groups())
    want = [p for d in (net.spec_spat_decoder, net.spec_decoder, net.spat_decoder) for p in d.parameters()]
    assert [id(p) for p in groups["decoder"]] == [id(p) for p in want]
    assert sum(len(g) for g in groups.values()) == len(list(net.parameters()))
    # pretrain=True wins over the flag, as in the reference (code/model.py:458, :470)
    both = model.SARSSL(sig_shape=(256, 8, 2, 2), pretrain=True, pretrain_frozen_encoder=True, device="cpu")
    assert hasattr(both, "decoder") and not hasattr(both, "spec_spat_decoder")


def test_frozen_model_rejects_cpu_input_and_use_cls():
    from sar_ssl_amd import model
    from sar_ssl_amd._lib import SarsslHipError
    net = model.SARSSL(sig_shape=(256, 8, 2, 2), pretrain=False, pretrain_frozen_encoder=True, device="cpu")
    with pytest.raises(SarsslHipError):
        net(torch.zeros((1, 2, 256, 8, 2)))
    with pytest.raises(NotImplementedError):
        model.SARSSL(sig_shape=(256, 8, 2, 2), pretrain=False, pretrain_frozen_encoder=True, use_cls=True, device="cpu")


def test_frozen_stage_flat_params_on_the_cpu_cover_the_three_decoders():
    from sar_ssl_amd import model, runtime
    net = model.SARSSL(sig_shape=(256, 8, 2, 2), pretrain=False, pretrain_frozen_encoder=True, device="cpu")
    flat = runtime.FlatParams(net)
    s, e = flat.group_spans["decoder"]
    assert e == flat.numel
    n = sum((p.numel() + 7) // 8 * 8 for d in (net.spec_spat_decoder, net.spec_decoder, net.spat_decoder) for p in d.parameters())
    assert e - s == n
    for k, p in net.named_parameters():
        if "encoder" in k:
            p.requires_grad = False
    fr = flat.frozen_ranges()
    assert fr == [(0, s)]                                                         # everything in front of the decoders, nothing of them


def test_command_line_and_directories():
    from sar_ssl_amd.opt import opt_pretrain
    o = opt_pretrain()
    args = o.parse(["--pretrain-frozen-encoder", "--simu-exp", "--time", "t0", "--work-dir", "/tmp/w", "--gpu-id", "0,"])
    assert args.pretrain_frozen_encoder and not args.pretrain and not args.test and args.simu_exp
    d = o.dir()
    assert d["log_pretrain_frozen_encoder"] == "/tmp/w/SAR-SSL/exp/pretrain_frozen_encoder/t0"
    assert d["log_pretrain"] == "/tmp/w/SAR-SSL/exp/pretrain/t0"
    import contextlib
    import io
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), pytest.raises(SystemExit):
        o.parse(["--help"])
    assert "not implemented" not in buf.getvalue() and "--pretrain-frozen-encoder" in buf.getvalue()
    with pytest.raises(AssertionError):
        opt_pretrain().parse(["--pretrain-frozen-encoder", "--pretrain", "--simu-exp"])


def test_more_than_one_gpu_id_is_refused_before_any_rank_is_spawned(monkeypatch):
    import sar_ssl_amd.run_pretrain as rp
    from sar_ssl_amd import launch
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(launch, "spawn_ranks", lambda *a, **k: pytest.fail("a rank was spawned"))
    with pytest.raises(SystemExit) as e:
        rp.main(["--pretrain-frozen-encoder", "--simu-exp", "--gpu-id", "0,1", "--work-dir", "/tmp/w", "--time", "t0"])
    assert "one GPU" in str(e.value)


def test_probe_inputs_restated_in_numpy_equal_what_the_reference_fed_its_encoders():
    z = _f17()
    gen = _generator()
    x = gen.probe_x()
    idx, ch = z["probe.mask_idx"], z["probe.mask_ch"]
    assert x.shape[0] == 3 and x.shape[3] == 8 and set(ch.tolist()) == {0, 1}
    spec, spat = probe_inputs_np(x, idx, ch)
    assert np.array_equal(spec, z["probe.spec_in"]) and np.array_equal(spat, z["probe.spat_in"])
    # what sets the stage apart from pretraining: nothing of the masked channel, nothing at the visible frames
    for b in range(3):
        vis = np.setdiff1d(np.arange(8), idx[b])
        s = spec[b].reshape(-1, 8, 2, 2)                                          # (F, T, reim, mic)
        assert not s[:, vis].any() and not s[:, :, :, ch[b]].any() and s[:, idx[b]][:, :, :, 1 - ch[b]].any()


def test_f17_loss_recomputed_with_the_reference():
    import ref_shim
    if not ref_shim.available():
        pytest.skip("reference tree not present")
    ref_model, ref_learner, _ = ref_shim.load()
    z = _f17()
    gen = _generator()
    net, loss, diff, vis, _ = gen.f17_step(ref_model, ref_learner)
    assert abs(loss.item() / float(z["loss"]) - 1) < 1e-6
    assert diff.item() == 0.0 and float(z["diff"]) == 0.0
    idx, ch = gen.masks_of(vis["mask"])
    assert np.array_equal(idx, z["mask_idx"]) and np.array_equal(ch, z["mask_ch"]) and set(ch.tolist()) == {0, 1}
    nograd = [k for k, p in net.named_parameters() if p.grad is None]
    assert nograd == json.loads(str(z["nograd_json"]))
    assert all(("encoder" in k) or k.startswith(("spec_decoder.", "spat_decoder.")) for k in nograd)


def test_one_epoch_schedule_is_its_warm_up_epoch():
    """`--nepoch 1` (what the entry-point test of this stage runs): the cosine schedule's only epoch is its warm-up epoch - the base rate,
    no division by the zero epochs behind it; longer schedules are what they were."""
    from sar_ssl_amd.common.utils import create_learning_rate_schedule
    one = create_learning_rate_schedule(total_steps=1, base=1e-3, decay_type="cosine", warmup_steps=1, linear_end=1e-6)
    assert float(one(1)) == pytest.approx(1e-3, rel=1e-6)
    two = create_learning_rate_schedule(total_steps=2, base=1e-3, decay_type="cosine", warmup_steps=1, linear_end=1e-6)
    assert float(two(1)) == pytest.approx(1e-3, rel=1e-6) and abs(float(two(2))) < 1e-9
