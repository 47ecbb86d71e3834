"""GPU: the fused Adam kernels (csrc/elementwise.hip adam_kernel / adam_dev_kernel) against a plain f64 restatement of the reference's
optimizer, torch.optim.Adam(lr, betas=(0.9, 0.999), eps=1e-8) without weight decay (code/learner.py:83).

All four entry points: hip.adam_step (the eager FusedAdam) and hip.adam_step_dev (the captured step; count and bias corrections in the
device step state), each with and without the hybrid mode's lo shadow.  New random gradients every step, gscale != 1, parameters from
1e-6 to 1e3 (lo parts in fp16's subnormal range, hi parts large), sizes that leave partial workgroups and one past the grid cap (the
grid-stride loop runs twice), a step whose guard is not finite, a zero_grad pass and a learning-rate change through an optimizer reset."""
import numpy as np
import pytest
import torch

from conftest import check

pytestmark = pytest.mark.gpu

BETAS, EPS = (0.9, 0.999), 1e-8
GSCALE = 0.37
LR0, LR1 = 1e-3, 3e-4
NSTEPS, SKIP_AT, RESET_AT = 8, 2, 5            # step SKIP_AT: guard = nan; step RESET_AT: a new optimizer (moments and count restart, LR1)
SIZES = [1, 3, 255, 257, 1000, 256 * 8192 + 5]    # (the launch caps the grid at 8192 workgroups of 256)
ENTRY = ["host", "host_lo", "dev", "dev_lo"]


def _f32(x):
    return float(np.float32(x))


def _ref_adam(p0, grads, plan, betas):
    """f64 torch.optim.Adam, one entry of ``plan`` per call: (t, lr, skipped, reset) - t = the bias-correction step the caller uses,
    reset = moments cleared in front of the call (a freshly constructed optimizer)."""
    b1, b2 = betas
    p = p0.clone()
    m = torch.zeros_like(p)
    v = torch.zeros_like(p)
    for g, (t, lr, skipped, reset) in zip(grads, plan):
        if reset:
            m.zero_()
            v.zero_()
        if skipped:
            continue
        g = g * _f32(GSCALE)
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        mh = m / (1 - b1 ** t)
        vh = v / (1 - b2 ** t)
        p = p - lr * mh / (vh.sqrt() + EPS)
    return p, m, v


def _shadows_ok(p, p16, ph16, pl16):
    """The shadows bit for bit against torch's conversions of the kernel's own parameters."""
    pc = p.cpu()
    assert torch.equal(p16.cpu(), pc.bfloat16())
    assert torch.equal(ph16.cpu(), pc.half())
    if pl16 is not None:
        assert torch.equal(pl16.cpu(), (pc - pc.half().float()).half())


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("entry", ENTRY)
def test_adam_entry_points_vs_f64_torch_adam(entry, n):
    from sar_ssl_amd import hip
    dev = torch.device("cuda:0")
    dev_path, with_lo = entry.startswith("dev"), entry.endswith("_lo")
    gen = torch.Generator().manual_seed(1000 + n + 7 * ENTRY.index(entry))
    sign = lambda: torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0).double()
    p0 = (sign() * 10.0 ** (-6.0 + 9.0 * torch.rand(n, generator=gen, dtype=torch.float64))).float()        # |p| in [1e-6, 1e3]
    # per element gradient scales from 1e-9 (sqrt(v) far below eps) to 1e2, new values every step
    gmag = 10.0 ** (-9.0 + 11.0 * torch.rand(n, generator=gen, dtype=torch.float64))
    grads = [(torch.randn(n, generator=gen, dtype=torch.float64) * gmag).float() for _ in range(NSTEPS)]

    p = p0.to(dev)
    g = torch.empty(n, device=dev)
    m = torch.zeros(n, device=dev)
    v = torch.zeros(n, device=dev)
    p16 = torch.zeros(n, dtype=torch.bfloat16, device=dev)
    ph16 = torch.zeros(n, dtype=torch.float16, device=dev)
    pl16 = torch.zeros(n, dtype=torch.float16, device=dev) if with_lo else None
    guard = torch.ones(1, device=dev)
    nskipped = torch.zeros(1, dtype=torch.int32, device=dev)
    st = hip.step_state_new(dev, 0x1234, LR0, BETAS) if dev_path else None

    plan, t_host, t_dev, lr = [], 0, 0, LR0
    for k in range(NSTEPS):
        skipped, reset = k == SKIP_AT, k == RESET_AT
        if reset:                                    # what PretrainStepGraph.reset_epoch / a new FusedAdam do
            lr, t_host, t_dev = LR1, 0, 0
            m.zero_()
            v.zero_()
            if dev_path:
                hip.step_state_reset(st, LR1, BETAS)
        g.copy_(grads[k].to(dev))
        guard.fill_(float("nan") if skipped else 1.0)
        before = [t.clone() for t in (p, m, v, p16, ph16) + ((pl16,) if with_lo else ())]
        zero_grad = k % 2 == 0 or skipped
        if dev_path:
            hip.step_tick(st)
            hip.adam_step_dev(p, g, m, v, p16, st, gscale=GSCALE, eps=EPS, zero_grad=zero_grad, ph16=ph16, guard=guard, pl16=pl16)
            if not skipped:
                t_dev += 1                           # a skipped step is not an optimizer step (GradScaler): the device count is taken back
            t = t_dev
        else:
            t_host += 1                              # FusedAdam.step: the host count advances on a skipped step as well (runtime.py)
            hip.adam_step(p, g, m, v, p16, lr, t_host, gscale=GSCALE, betas=BETAS, eps=EPS, ph16=ph16,
                          guard=None if k == 0 else guard, nskipped=None if k == 0 else nskipped, pl16=pl16)
            t = t_host
        torch.cuda.synchronize()
        plan.append((t, lr, skipped, reset))
        after = (p, m, v, p16, ph16) + ((pl16,) if with_lo else ())
        if skipped:
            assert all(torch.equal(a, b) for a, b in zip(after, before)), "a skipped step moved parameters, moments or shadows"
        else:
            assert not torch.equal(p, before[0]) or n == 1
        if dev_path:
            assert bool((g == 0).all()) if zero_grad else torch.equal(g.cpu(), grads[k]), "zero_grad=%d" % zero_grad
        else:
            assert torch.equal(g.cpu(), grads[k])    # the host-count kernel never clears the gradient
        _shadows_ok(p, p16, ph16, pl16)

    assert (hip.step_state_skipped(st) if dev_path else int(nskipped.item())) == 1

    # f64 restatement.  The kernels receive the betas as f32 (c_float): the moments are checked against the same recursion with those
    # values (1 - f32(0.999) is 1.3e-5 away from 0.001 relative, and the bias correction 1 - f32(0.999)^t follows it, so the update
    # stays that of betas (0.9, 0.999)); the update is checked against the exact betas as well.
    b32 = (_f32(BETAS[0]), _f32(BETAS[1]))
    p0d = p0.double()
    pr, mr, vr = _ref_adam(p0d, [gr.double() for gr in grads], [(t, _f32(lr_), s, r) for t, lr_, s, r in plan], b32)
    pr_exact, _, _ = _ref_adam(p0d, [gr.double() for gr in grads], plan, BETAS)
    _, mabs, _ = _ref_adam(p0d, [gr.double().abs() for gr in grads], [(t, _f32(lr_), s, r) for t, lr_, s, r in plan], b32)
    pk = p.cpu().double()
    # update error relative to the update's largest magnitude; the parameters are stored in f32, so each step may also round p by half a
    # unit in the last place of |p| (up to 3e-5 at 1e3, where the whole update is ~5e-3): that slack is granted per element
    slack = 0.5 * NSTEPS * torch.from_numpy(np.spacing(np.maximum(p0.abs().numpy(), p.abs().cpu().numpy()))).double()
    for name, want in (("f32betas", pr), ("torch", pr_exact)):
        upd = want - p0d
        err = ((pk - p0d) - upd).abs()
        check("adam.%s.n%d.update.%s" % (entry, n, name), float((err - slack).clamp_min(0).max() / upd.abs().max()), 1e-5)
    # moments: v per element; m per element against the same recursion on |g| (m itself may cancel to ~0)
    check("adam.%s.n%d.m" % (entry, n), float(((m.cpu().double() - mr).abs() / mabs.clamp_min(1e-30)).max()), 1e-6)
    check("adam.%s.n%d.v" % (entry, n), float(((v.cpu().double() - vr).abs() / vr.clamp_min(1e-38)).max()), 1e-6)
    if with_lo and n >= 255:                         # the lo shadows do reach fp16's subnormal range (and were not flushed)
        lo = pl16.float().abs()
        assert bool(((lo > 0) & (lo < 2.0 ** -14)).any())


@pytest.mark.parametrize("with_lo", [False, True])
def test_adam_step_dev_without_a_guard_is_the_step_behind_a_finite_guard(with_lo):
    """sarssl_adam_step_dev with guard = NULL (a caller that never skips) against the same launch behind a finite guard, which the test
    above pins: parameters, moments, shadows and the cleared gradient bit for bit; n = 1000 leaves a partial workgroup."""
    from sar_ssl_amd import hip
    dev = torch.device("cuda:0")
    n = 1000
    gen = torch.Generator().manual_seed(77)
    p0 = torch.randn(n, generator=gen)
    g0 = torch.randn(n, generator=gen) * 1e-2
    results = []
    for guard in (torch.ones(1, device=dev), None):
        p, g = p0.to(dev), g0.to(dev)
        m, v = torch.full((n,), 1e-3, device=dev), torch.full((n,), 1e-6, device=dev)
        p16 = torch.zeros(n, dtype=torch.bfloat16, device=dev)
        ph16 = torch.zeros(n, dtype=torch.float16, device=dev)
        pl16 = torch.zeros(n, dtype=torch.float16, device=dev) if with_lo else None
        st = hip.step_state_new(dev, 0x1234, LR0, BETAS)
        hip.step_tick(st)
        hip.adam_step_dev(p, g, m, v, p16, st, gscale=GSCALE, eps=EPS, zero_grad=True, ph16=ph16, guard=guard, pl16=pl16)
        torch.cuda.synchronize()
        assert hip.step_state_skipped(st) == 0 and bool((g == 0).all()) and not torch.equal(p.cpu(), p0)
        _shadows_ok(p, p16, ph16, pl16)
        results.append((p, m, v, p16, ph16) + ((pl16,) if with_lo else ()))
    assert all(torch.equal(a, b) for a, b in zip(*results))
