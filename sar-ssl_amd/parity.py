"""Parity class of every numeric mode: the gates that tests/ ASSERT against the reference's golden vectors on MI355X, in one place so
that bench.py's `parity_class` prints exactly what is asserted (round-3 verdict: the line claimed 1e-2 per bin while the test gate
was 3e-2).  north_star: "within 1e-3 relative on the reconstruction loss and per-bin magnitudes ... 100-step recon-loss curve within
1e-3 of reference".

Quantities (fixture F3, tests/test_gpu_model.py::test_fullsize_forward_backward; F5 / F12, tests/test_gpu_train.py):
  loss          |loss / loss_ref - 1|, full-size forward, eval and train mode
  per_bin_max   max over F3's 2 048 sampled `pred` bins of |pred - pred_ref| / max|pred_ref|
  per_bin_rms   rms of the same deviations / max|pred_ref|
  grad_norm     worst per-parameter gradient L2 norm, relative
  bn_running    BatchNorm running statistics after one train-mode forward
  curve100      max relative deviation of the 100-step loss curve (dropout off, replayed masks)
`measured` = what the MI355X run of round 4 measured (eval / train), for the reader; gates sit at <= 5x measured and never above the
class the mode claims.

Round 5, per_bin_max of the timed mode: it sits AT north_star's 1e-3, not inside it - 9.1e-4 in eval mode, 1.21e-3 in train mode (maximum
of 2 048 bins whose rms deviation is 2-3e-4 of range), gated at 1.5e-3 and stated so in `parity_class`.  A two-pass fp16 split of a SUBSET of
the contractions does not change that (profiles/r05_operand_rounding_study.txt: decoder in f32 - eval 6.5e-4 but train 1.12e-3; every
Conformer Linear in f32 operands AND f32 storage - 6.3e-4 / 7.7e-4; with 16-bit activation storage no family subset moves the train-mode
rms of 3.1e-4): the deviation is the fp16 rounding of the STORED activations between layers, amplified by the train-mode BatchNorm
statistics, not the operand rounding of a few products.  Inside 1e-3 with margin costs f32 storage (`fp32`, 61 ms).  What the timed mode
claims: loss / curve / rms inside 1e-3, per-bin maximum 1.5e-3.
"""

GATES = {
    # round 6 - fp16 CNN stem + f32 residual stream in the Conformer blocks / decoder (f32 activations and weights as fp16 pairs on the
    # matrix cores): the mode that meets north_star's 1e-3 per bin at 16-bit matrix-core speed
    # grad_norm: worst parameter overall - always one whose gradient is a near-cancelling sum formed by the bf16 backward pass (BatchNorm
    # betas of the stem, the attention module's u / v biases: measured 0.7-1.1e-2 on F3 / F14, same as the fp16 mode's); grad_norm_body: the
    # parameters outside the stem and those biases, whose gradients flow along the f32 stream (measured 2.1e-3 on F14 / F3 eval, 3.4e-3 F3 train, <= 4.5e-3 on F15; fp16 mode: 1.7e-2)
    "hybrid": dict(loss=1e-3, per_bin_max=1e-3, per_bin_rms=3e-4, grad_norm=1.5e-2, grad_norm_body=5e-3, bn_running=5e-4, curve100=1e-3,
                   measured=dict(loss=(1.1e-6, 1.0e-6), per_bin_max=(3.3e-4, 8.5e-4), per_bin_rms=(7.6e-5, 2.2e-4), grad_norm=(1.03e-2, 9.6e-3),
                                 grad_norm_body=(2.1e-3, 3.4e-3), curve100=1.9e-4,
                                 b64_f13=dict(per_bin_max=(2.6e-4, 6.5e-4), per_bin_rms=(7.0e-5, 1.6e-4)))),
    # fp16 forward / bf16 backward - the mode bench.py times since round 4
    "fp16": dict(loss=1e-3, per_bin_max=1.5e-3, per_bin_rms=5e-4, grad_norm=2.5e-2, bn_running=5e-4, curve100=1e-3,
                 measured=dict(loss=(6.1e-6, 9.6e-7), per_bin_max=(9.1e-4, 1.21e-3), grad_norm=(1.5e-2, 7.9e-3), curve100=1.9e-4)),
    # bf16 throughout - the timed mode of rounds 1-3
    "bf16": dict(loss=2e-3, per_bin_max=3e-2, per_bin_rms=1e-2, grad_norm=6e-2, bn_running=5e-3, curve100=1e-3,
                 measured=dict(loss=(3.8e-4, 1.2e-4), per_bin_max=(5.8e-3, 1.1e-2), grad_norm=(2.3e-2, 3.5e-2), curve100=1.6e-4)),
    # f32 storage, every contraction as three split-bf16 MFMA passes
    "fp32": dict(loss=1e-3, per_bin_max=1e-3, per_bin_rms=1e-3, grad_norm=5e-3, bn_running=1e-4, curve100=1e-3,
                 measured=dict(loss=(2.3e-7, 2.4e-7), per_bin_max=(9.7e-6, 1.5e-5), grad_norm=(3.5e-4, 3.9e-4), curve100=1.9e-4)),
    # f32 storage, one bf16 MFMA pass (round-3 experiment)
    "fp32_1pass": dict(loss=2e-3, per_bin_max=3e-2, per_bin_rms=1e-2, grad_norm=6e-2, bn_running=5e-3, curve100=None, measured=dict()),
}

# The RIR renderer (csrc/rirmix.hip) against the f64 numpy / scipy restatement of an item (rirsynth.restate_*), max |difference| of the
# peak-normalised outputs = error relative to full scale (tests/test_gpu_rirmix.py).  cap: half a PCM-16 step, the quantisation the
# simulated branch's stored segments already carry - a condition, not a measurement.  gate: 4x the largest distance measured on an MI355X
# over the test's shapes, rounded up to one digit (profiles/rirmix.txt).
# restatement_vs_f20: the same distance between the f64 restatement and fixture F20 of the real reference (mixed f32 / f64 arithmetic, stored
# as f32), measured on the CPU (tests/test_rirsynth_cpu.py prints it), x4, one digit; the renderer is held to gate + restatement_vs_f20
# against F20 (triangle inequality).
# The stored direct-path signal (sarssl_rir_mix_dp's out_dp, tests/test_gpu_simsig_dp.py) is held to the same gate as out - the same
# transforms over fewer partitions - and restate_sig(with_dp=True) against fixture F24 of the real reference to restatement_vs_f20 - the
# same two fftconvolve calls (tests/test_simsig_dp_cpu.py); rir_mix_dp and restatement_dp_vs_f24 record what those tests measure.
# realsig.restate_item (the measured variant at gain 0.9, the generator of gen_sig_from_real_rir.py) is held to restatement_vs_f20 against
# fixture F26 of the real reference's MicSigFromRIRDataset (tests/test_realsig_cpu.py); restatement_vs_f26 records what it measures.
RIRMIX = dict(gate=2e-6, cap=1.5e-5, restatement_vs_f20=8e-7,
              measured=dict(rir_mix=2.8e-7, diffuse_noise=2.9e-7, loader=3.1e-7, restatement_vs_f20=1.9e-7, rir_mix_dp=2.7e-7,
                            restatement_dp_vs_f24=7.5e-9, restatement_vs_f26=1.5e-7))


# The image-source renderer (csrc/ism.hip) against the f64 numpy restatement roomsim.restate_ism: max |difference| over an RIR relative to
# the RIR's absolute peak (tests/test_gpu_ism.py).  cap: half a PCM-16 step of full scale, as for RIRMIX - a condition, not a measurement.
# gate: 4x the largest distance measured on an MI355X over the test's shapes, rounded up to one digit (profiles/ism.txt).  t60_gate: the same
# for |T60_edc(GPU RIR) - T60_edc(restatement)| in seconds; t60_cap 5e-3 s, a tenth of the window the reference's accept test allows.
# (tools/bench_ism.py measures 4.9e-7 over rooms idx 0..7 of stage train: rooms with more images than the test's two sit closer to the gate.)
ISM = dict(gate=7e-7, cap=1.5e-5, t60_gate=7e-8, t60_cap=5e-3,
           measured=dict(ragged=1.4e-7, tail=1.4e-7, full_size=1.5e-7, direct_path=1.3e-7, t60_edc=1.6e-8))

# The labels kernel (csrc/rirlabel.hip: sarssl_rir_labels) against roomsim.labels on identical f32 input (tests/test_gpu_simsig.py):
# largest |device - host| of the per-channel T60 in seconds, of the fit's correlation, of DRR and of C50 in dB, over the synthetic cases
# of tests/simsig_cases.py at 1, 2 and 3 channels.  Both sides are f64; they differ in the order of the sums and in the closed-form fits
# from centred suffix sums instead of scipy.stats.linregress per stretch.
#   cap       a condition, not a measurement: t60 = ISM's t60_cap (a tenth of the accept test's window; every test item sits at least
#             0.029 s inside it, so the decision cannot flip); DRR / C50 1e-3 dB, far below a float16 step at their magnitude; corr 1e-9 -
#             what the cancellation in sum y^2 - (sum y)^2 / N can cost at most: N 2^-53 relative on sums below N 74^2 (E lies in
#             [-100, 0] dB, centred at -26) over a variance of at least 8 dB^2 (a 10 dB stretch) = 1e-9 at N = 14 000
#   measured  on an MI355X (profiles/simsig.txt)
#   gate      4x measured, rounded up to one digit; the tolerance of a test is min(gate, cap)
RIRLABELS = dict(cap=dict(t60=5e-3, corr=1e-9, drr=1e-3, c50=1e-3),
                 measured=dict(t60=1.5e-14, corr=3.5e-14, drr=3.6e-15, c50=1.8e-15),
                 gate=dict(t60=6e-14, corr=2e-13, drr=2e-14, c50=8e-15))

# The signal generator (roomsim.simulate_signals) against roomsim.restate_sig of the same plan, in PCM-16 steps (tests/test_gpu_simsig.py).
#   pcm_step     derived, not measured: the mix gate RIRMIX['gate'] = 2e-6 of full scale is 0.066 of a PCM step, below one half, so the
#                rounded values differ by at most one step
#   share_bound  derived: a sample can differ only where the f64 value lies within the gate of a rounding boundary, a share of
#                2 gate 32767 = 0.131 of all samples
#   measured     the largest share of differing samples of an item on an MI355X (recorded, not gated below the bound)
SIMSIG = dict(pcm_step=1, share_bound=2 * RIRMIX["gate"] * 32767, measured=dict(share=3.3e-3, max_step=1))

# The mixing-table kernel (csrc/rirmix.hip: sarssl_mixing_table) against rirsynth.mixing_table(...).astype(float32): max |device - host|
# over the geometries of tests/certainroom_cases.py at B = 1 and B = 5 (tests/test_gpu_certainroom.py).  Both sides factor in f64 and round
# to f32 once; they differ in the library's sin and in the order of the factorisation's sums.
#   cap       a condition, not a measurement: two f32 units at the entries' largest magnitude 1 (2^-22)
#   measured  on an MI355X (profiles/certainroom.txt)
#   gate      4x measured, rounded up to one digit, never above the cap; the tolerance of the test is min(gate, cap)
#             (0: the f32 tables are bit-identical for every geometry of the test, so the test asserts equality)
MIXTABLE = dict(cap=2.0 ** -22, measured=0.0, gate=0.0)

# The polyphase resampler (csrc/resample.hip) against the f64 numpy restatement realrir.restate_resample on the input as the kernel reads
# it: max |difference| of a case relative to the case's absolute peak (tests/test_gpu_resample.py).  Both sides use the same taps - the
# kernel their f32 rounding - and the same order of the sum; they differ in the f32 products and the f32 accumulator.
#   cap       a condition, not a measurement: half a PCM-16 step of full scale, as for RIRMIX
#   ceiling   the gate may not exceed RIRMIX's, the gate of the same kind of f32 sum
#   measured  on an MI355X over the test's cases (profiles/resample.txt, next to scipy's own float32 path on the same inputs)
#   gate      about 5x the largest measured distance, one digit, never above the ceiling (5 x 4.3e-7 = 2.2e-6 -> 2e-6); the tolerance of
#             a case is min(gate, ceiling, cap) x peak.  scipy's float32 path measures 2.1 - 4.3e-7 on the same inputs
RESAMPLE = dict(cap=1.5e-5, ceiling=2e-6, measured=dict(kernel=4.3e-7, scipy_f32=4.3e-7, realrir_rir=1.6e-7, realrir_drr_db=2.6e-6,
                                                         realrir_c50_db=1.7e-6), gate=2e-6)

# The LOCATA TDOA corpus (locatads.py, csrc/locata.hip).
#   label / signal    locatads.TdoaCorpus.restate_item against the reference's LOCATADataset.__getitem__ over the items of fixture F27
#                     (tests/test_locatads_cpu.py).  The label: |float32(restatement) - reference's float32 label| relative to the label's
#                     magnitude; both sides form the same f64 expressions in numpy, measured 0 on all 24 items, so the gate is 0 (equality)
#                     and the cap, a condition, is one float32 unit (2^-23).  The signal: max |restatement - reference| relative to the
#                     item's peak 0.9 - the reference resamples in float32 (scipy keeps the input's dtype), the restatement in f64;
#                     measured 3.5e-7, the gate 4x that, under RESAMPLE's ceiling
#   interp_mean       hip.interp_mean against np.interp(...).mean(axis=0) in f64 (tests/test_gpu_locatads.py): |difference| relative to the
#                     column's largest |value|.  Same values term by term; numpy sums pairwise, the kernel in runs of ceil(n / 256) and
#                     then over 256 partials.  ulps: the gate in units of 2^-52 log2(max(n, 2)) - "a few f64 ulp times log2(n)";
#                     measured: the largest distance seen in those units on an MI355X
#   peak_scale        hip.peak_scale against numpy in f32, operation for operation (max|x|; 0.9f / (peak + 1e-8f); one product per
#                     sample): the peak and - measured - the scaled samples are bit-equal, so the gate is 0 (equality); cap: one float32
#                     unit of the item's peak 0.9
#   generate          the files of locatads.generate against restate_item: half a PCM-16 step plus RESAMPLE's gate at full scale, in
#                     PCM-16 steps; the labels (float32) against float32(restate_item's): the kernel's gate in f64 moves a float32
#                     rounding only where the f64 value sits on a boundary, so one float32 unit
LOCATADS = dict(label=dict(cap=2.0 ** -23, measured=0.0, gate=0.0), signal=dict(ceiling=RESAMPLE["ceiling"], measured=3.5e-7, gate=1.4e-6),
                interp_mean=dict(ulps=4.0, measured=3.3), peak_scale=dict(cap=2.0 ** -23, measured=0.0, gate=0.0),
                generate=dict(pcm_steps=0.5 + RESAMPLE["gate"] * 32767, label=2.0 ** -23, measured=dict(pcm_steps=0.511, label=0.0)))

# The row / elementwise kernels (csrc/elementwise.hip, the row kernels of csrc/dwconv.hip, csrc/head.hip) against the f64 restatements of
# tests/rowkernel_refs.py on the operands as stored: max |got - ref| / max |ref| (tests/test_gpu_rowkernels.py).  Keyed by kernel family,
# then by the storage dtype of a forward kernel or the (gradient, saved activation) pairing of a backward kernel: f32, bf16, fp16,
# mix16 = (bf16, fp16), mixf32 = (bf16, f32).
#   cap           a condition, not a measurement: two units in the last place of the OUTPUT dtype at the reference's largest magnitude
#                 (bf16 2^-7, fp16 2^-10, f32 2^-22) - one rounding from f32 arithmetic on the stored operands stays inside, a 16-bit
#                 intermediate does not
#   cap_per_term  f32 outputs that are sums: 2^-23 per addend, L addends -> L * 2^-23.  dgamma / dbeta (L = rows), column sums and means,
#                 weight gradients (L = B * T), the small Linear layers, and - what an f32 accumulation of that many terms cannot be held
#                 to 2 ulp for - the depthwise convolutions' outputs (L = 31 taps: dwconv_fwd, dwglu_fwd, dwglu_bwd measure 2.5 - 2.7e-7 in
#                 f32, 2^-22 is 2.4e-7) and the softmax rows (L = T: the normalising sum, and exp turns the two roundings of a score of
#                 magnitude s into a relative error of s * 2^-23: 2.8e-7 at T = 1024).  An addend is a term of the sum, the value already
#                 in a `+=` destination and a bias included, so that a one-term `+=` is held to the elementwise f32 cap
#   dwglu_wgrad   bf16 / mix16: the kernel recomputes g = GLU(h) AS STORED (rounded to h's 16-bit dtype, csrc/dwconv.hip as_stored, so
#                 that the fused and the unfused path agree), the reference rounds its f64 g the same way, and an f32 sigmoid lands on
#                 the other side of a rounding boundary for about one g in 2 500 (fp16): one addend moves by a 16-bit ulp.  Cap = 2 ulp
#                 of that dtype; the f32 pairing has no such rounding and is held to L * 2^-23
#   gate          4x the largest deviation measured on an MI355X over the test's shapes, rounded up to one digit, never above the cap
#                 (profiles/rowkernels.txt is the run); the tolerance of a case is min(gate, cap)
_E32, _EBF, _EFP, _PER = 2.0 ** -22, 2.0 ** -7, 2.0 ** -10, 2.0 ** -23


def _rk(cap, measured, gate):
    return dict(cap=cap, measured=measured, gate=gate)


def _rs(measured, gate):
    return dict(cap_per_term=_PER, measured=measured, gate=gate)


ROWKERNELS = {
    "ln_fwd": {"f32": _rk(_E32, 1.43e-7, _E32), "bf16": _rk(_EBF, 3.20e-3, _EBF), "fp16": _rk(_EFP, 3.69e-4, _EFP)},
    "ln_fwd_stats": {"f32": _rs(1.05e-7, 5e-7), "bf16": _rs(1.14e-7, 5e-7), "fp16": _rs(1.13e-7, 5e-7)},
    "ln_bwd_dx": {"f32": _rk(_E32, 1.09e-7, _E32), "bf16": _rk(_EBF, 3.36e-3, _EBF), "mix16": _rk(_EBF, 3.34e-3, _EBF),
                  "mixf32": _rk(_EBF, 3.34e-3, _EBF)},
    "ln_bwd_dparam": {"f32": _rs(1.95e-7, 8e-7), "bf16": _rs(1.88e-7, 8e-7), "mix16": _rs(1.86e-7, 8e-7), "mixf32": _rs(1.60e-7, 7e-7)},
    "glu_fwd": {"f32": _rk(_E32, 7.86e-8, _E32), "bf16": _rk(_EBF, 2.44e-3, _EBF), "fp16": _rk(_EFP, 3.06e-4, _EFP)},
    "glu_bwd": {"f32": _rk(_E32, 1.42e-7, _E32), "bf16": _rk(_EBF, 2.11e-3, _EBF), "mix16": _rk(_EBF, 2.02e-3, _EBF),
                "mixf32": _rk(_EBF, 2.02e-3, _EBF)},
    "dwconv_fwd": {"f32": _rs(2.52e-7, 2e-6), "bf16": _rk(_EBF, 3.68e-3, _EBF), "fp16": _rk(_EFP, 4.50e-4, _EFP)},
    "dwconv_wgrad": {"f32": _rs(2.15e-7, 9e-7), "bf16": _rs(1.59e-7, 7e-7), "mix16": _rs(1.60e-7, 7e-7), "mixf32": _rs(2.16e-7, 9e-7)},
    "dwglu_fwd": {"f32": _rs(2.63e-7, 2e-6), "bf16": _rk(_EBF, 3.12e-3, _EBF), "fp16": _rk(_EFP, 4.15e-4, _EFP)},
    "dwglu_bwd": {"f32": _rs(2.69e-7, 2e-6), "bf16": _rk(_EBF, 3.44e-3, _EBF), "mix16": _rk(_EBF, 3.43e-3, _EBF)},
    "dwglu_wgrad": {"f32": _rs(2.47e-7, 1e-6), "bf16": _rk(_EBF, 2.76e-7, 2e-6), "mix16": _rk(_EFP, 8.34e-5, 4e-4)},
    "softmax_fwd": {"f32": _rs(2.83e-7, 2e-6), "bf16": _rk(_EBF, 3.37e-3, _EBF), "fp16": _rk(_EFP, 4.02e-4, _EFP)},
    "softmax_bwd": {"f32": _rs(2.25e-7, 1e-6), "bf16": _rk(_EBF, 3.21e-3, _EBF), "mix16": _rk(_EBF, 3.10e-3, _EBF),
                    "mixf32": _rk(_EBF, 3.13e-3, _EBF)},
    "bias2": {"f32": _rk(_E32, 5.08e-8, _E32), "bf16": _rk(_EBF, 3.55e-3, _EBF), "fp16": _rk(_EFP, 3.93e-4, _EFP)},
    "axpby": {"f32": _rk(_E32, 4.42e-8, 2e-7), "bf16": _rk(_EBF, 2.90e-3, _EBF), "fp16": _rk(_EFP, 3.62e-4, _EFP)},
    "axpby2d": {"f32": _rk(_E32, 5.79e-8, _E32), "bf16": _rk(_EBF, 3.03e-3, _EBF), "fp16": _rk(_EFP, 3.79e-4, _EFP)},
    "act_bwd": {"f32": _rk(_E32, 1.29e-7, _E32), "bf16": _rk(_EBF, 2.45e-3, _EBF), "mix16": _rk(_EBF, 2.52e-3, _EBF),
                "mixf32": _rk(_EBF, 2.50e-3, _EBF)},
    "f64_accum": {"f32": _rk(_E32, 7.97e-8, _E32)},
    "colsum_store": {"f32": _rs(4.05e-7, 2e-6), "bf16": _rk(_EBF, 3.15e-3, _EBF), "fp16": _rk(_EFP, 4.35e-4, _EFP)},
    "colsum": {"f32": _rs(1.80e-7, 8e-7), "bf16": _rs(1.43e-7, 6e-7), "fp16": _rs(2.06e-7, 9e-7)},
    "bn_eval_affine": {"f32": _rk(_E32, 9.24e-8, _E32)},
    "mean_rows": {"f32": _rs(5.89e-7, 3e-6), "bf16": _rs(5.47e-8, 3e-7), "fp16": _rs(9.84e-8, 4e-7)},
    "mean_rows_bwd": {"f32": _rk(_E32, 5.13e-8, _E32), "bf16": _rk(_EBF, 2.85e-3, _EBF)},
    "small_linear_fwd": {"f32": _rs(9.87e-8, 4e-7)},
    "small_linear_bwd": {"f32": _rs(3.63e-7, 2e-6)},
}


def rowkernel_tol(family, key, L=None):
    """Tolerance tests/test_gpu_rowkernels.py asserts for one case: the family's gate, never above the cap (L: addends of a sum)."""
    e = ROWKERNELS[family][key]
    cap = e["cap"] if "cap" in e else L * e["cap_per_term"]
    return min(e["gate"], cap)


# The GEMM family (csrc/gemm.hip, csrc/gemm_epilogue.h: sarssl_gemm, sarssl_gemm_split, sarssl_gemm_group_tn) against the f64 restatement
# of tests/gemm_refs.py on the operands as stored and as staged (the fp16 -> bf16 re-encoding of the mixed pairings, the bf16 rounding of
# the f32 fast mode, the hi / lo parts of the precise mode and of the fp16 pairs): max |got - ref| / max |ref| (tests/test_gpu_gemm.py).
# Keyed by family - product (C), preact (the saved pre-activation), actbwd (C of a fused activation backward), splitk (C += alpha A B, the
# grouped launch and its column sums included), pair (sarssl_gemm_split) - then by dtype triple (A, B, C): bf16, bf16_f32, fp16, fp16_f32,
# mix_ga = (bf16, fp16, bf16), mix_ga_f32, mix_ag = (fp16, bf16, bf16), f32_fast, f32_precise; pair: by C's dtype.  _gemm_family takes the
# measured figures and the gates below the cap per triple; a 16-bit C measures 0.33 - 0.42 of its cap (4x is above it), so its gate IS the cap.
#   cap           conditions, not measurements.  16-bit C: two units in the last place of the output dtype (bf16 2^-7, fp16 2^-10).  f32
#                 precise: the 5e-5 the suite has always asserted of the three split-bf16 passes.  pair, f32 C: the 3e-6 of
#                 tests/test_gpu_hybrid.py (fp16 C: 2 ulp of fp16 - a 16-bit output cannot be held to the contraction's 2^-21)
#   cap_per_term  f32 C from 16-bit operands or from the fast mode's bf16-rounded ones: L * 2^-23 with L = K + the epilogue's addends
#                 (bias, residual, the value already in C), and never above cap_max = 1e-5, what tests/test_gpu_kernels.py asserts of them
#   gate          4x the largest deviation measured on an MI355X over the cases of tests/test_gpu_gemm.py, rounded up to one digit, never
#                 above the cap (profiles/gemm.txt is the run); the tolerance of a case is min(gate, cap)
def _gs(measured, gate):
    return dict(cap_per_term=_PER, cap_max=1e-5, measured=measured, gate=gate)


_G16 = dict(bf16=_EBF, fp16=_EFP, mix_ga=_EBF, mix_ag=_EBF)


def _gemm_family(measured, gates, keys):
    out = {}
    for k in keys:
        m, g = measured.get(k), gates.get(k)
        if k in _G16:
            out[k] = _rk(_G16[k], m, _G16[k] if g is None else g)
        elif k == "f32_precise":
            out[k] = _rk(5e-5, m, 5e-5 if g is None else g)
        else:
            out[k] = _gs(m, 1e-5 if g is None else g)
    return out


_GEMM_ALL = ("bf16", "bf16_f32", "fp16", "fp16_f32", "mix_ga", "mix_ga_f32", "mix_ag", "f32_fast", "f32_precise")
_GEMM_ACC = ("bf16_f32", "fp16_f32", "mix_ga_f32", "f32_fast", "f32_precise")
GEMM = {
    "product": _gemm_family(dict(bf16=3.18e-3, bf16_f32=7.66e-7, fp16=4.03e-4, fp16_f32=1.38e-7, mix_ga=2.77e-3, mix_ga_f32=1.32e-7, mix_ag=2.78e-3,
                                 f32_fast=1.43e-7, f32_precise=1.25e-7),
                            dict(bf16_f32=4e-6, fp16_f32=6e-7, mix_ga_f32=6e-7, f32_fast=6e-7, f32_precise=5e-7), _GEMM_ALL),
    "preact": _gemm_family(dict(bf16=3.20e-3, bf16_f32=7.66e-7, fp16=4.03e-4, fp16_f32=1.05e-7, mix_ga=2.59e-3, mix_ga_f32=1.07e-7, mix_ag=2.60e-3,
                                f32_fast=9.18e-8, f32_precise=1.01e-7),
                           dict(bf16_f32=4e-6, fp16_f32=5e-7, mix_ga_f32=5e-7, f32_fast=4e-7, f32_precise=5e-7), _GEMM_ALL),
    "actbwd": _gemm_family(dict(bf16=3.15e-3, fp16=4.14e-4, bf16_f32=1.74e-7), dict(bf16_f32=7e-7), ("bf16", "fp16", "bf16_f32")),
    "splitk": _gemm_family(dict(bf16_f32=3.49e-7, fp16_f32=4.33e-7, mix_ga_f32=3.93e-7, f32_fast=3.49e-7, f32_precise=3.56e-7),
                           dict(bf16_f32=2e-6, fp16_f32=2e-6, mix_ga_f32=2e-6, f32_fast=2e-6, f32_precise=2e-6), _GEMM_ACC),
    "pair": {"fp16": _rk(_EFP, 3.72e-4, _EFP), "f32": _rk(3e-6, 2.99e-7, 2e-6)},
}


def gemm_tol(family, key, L=None):
    """Tolerance tests/test_gpu_gemm.py asserts for one case: the family's gate, never above the cap (L: K + the epilogue's addends)."""
    e = GEMM[family][key]
    cap = e["cap"] if "cap" in e else min(L * e["cap_per_term"], e["cap_max"])
    return min(e["gate"], cap)


def parity_class(precision):
    """What bench.py prints for the timed mode."""
    g = GATES[precision]
    return {"loss_vs_reference": g["loss"], "loss_curve_100_steps": g["curve100"], "per_bin_pred_of_range_max": g["per_bin_max"],
            "per_bin_pred_of_range_rms": g["per_bin_rms"], "per_parameter_grad_norm": g["grad_norm"], "measured_eval_train": g["measured"],
            "north_star": "1e-3 on the loss, the per-bin magnitudes and the 100-step curve",
            "meets_north_star": ({"loss": True, "curve100": True, "per_bin_rms": True,
                                  "per_bin_max": "NO in train mode: measured 9.1e-4 (eval) / 1.21e-3 (train) of range, gated at 1.5e-3 - the maximum over "
                                                 "2 048 bins of rounding noise with rms 2-3e-4; the fp32 mode measures 1.5e-5"}
                                 if g["per_bin_max"] > 1e-3 else {"loss": True, "curve100": g["curve100"] is not None, "per_bin_rms": True, "per_bin_max": True}),
            "pinned_by": "tests/test_gpu_model.py::test_fullsize_forward_backward (F3), tests/test_gpu_train.py (F5, F12), "
                         "tests/test_gpu_graph.py (B = 64 captured step vs the fp32 mode, F13 reference forward at B = 64)"}
