"""Wall time of the batched SDR suggest (qcqpmi_sdr_small_batch; --wide: qcqpmi_sdr_batch, n up to 128) against the per-problem loop
it replaces.

Workload: problems.boolean_least_squares_batch(B, n, m), S samples per problem; both paths at their own defaults (max_sweeps = 5000,
tol = 1e-11).
  batched    ONE call of Engine.sdr_small_batch (uploads of the B objectives, the launch, the downloads of y, primal, sweeps and the
             B S n samples) + sdr.certify_batch on the host (one batched eigvalsh): host clock around both, --repeat calls after one
             warm-up, median.  The certification's share is reported on its own.
  loop       what the library offered before: per problem QCQP(Problem).suggest(SDR, num_samples=S) -- a context, the lifted cost, one
             cooperative launch of sdr_mixing_kernel, V to the host, the certificate, an SVD for the sampling factor, the upload of mu
             and F, the sampling and evaluation launches.  Timed on the first --loop-problems problems and SCALED LINEARLY to B (every
             problem costs the same launches; stated as such in the output).
--wide: the batched call is Engine.sdr_batch, the entry point of QCQPBatch.suggest(SDR, wide=True) (n <= 64: the same launch; 65 <= n
<= 128: sdr_small_kernel<true>).  Without the flag the tool runs what it always ran.
Prints one JSON line (with how many of the timed problems both paths certify and the largest relative difference of their bounds).
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--B', type=int, default=4096)
    ap.add_argument('--n', type=int, default=32)
    ap.add_argument('--m', type=int, default=48)
    ap.add_argument('--S', type=int, default=64)
    ap.add_argument('--repeat', type=int, default=5)
    ap.add_argument('--loop-problems', type=int, default=64)
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--wide', action='store_true', help='Engine.sdr_batch (qcqpmi_sdr_batch): n up to 128')
    args = ap.parse_args()

    import numpy as np
    from qcqp_amd import QCQP, Problem, problems, sdr, settings as s
    from qcqp_amd.batch import QCQPBatch
    from qcqp_amd.engine import device_count
    if device_count() < 1:
        raise SystemExit('bench_sdr_batch: no HIP device visible (there is no CPU path)')

    fl = problems.boolean_least_squares_batch(args.B, args.n, args.m, seed=args.seed)
    qb = QCQPBatch(fl)
    e = qb.engine
    d = sdr.unit_diagonal_family(qb.form)
    C = sdr.lifted_cost_batch(qb.P0s, qb.q0s, qb.r0s, d)

    run = e.sdr_batch if args.wide else e.sdr_small_batch

    def batched():
        t0 = time.perf_counter()
        o = run(qb.P0s, qb.q0s, qb.r0s, args.S, seed=args.seed, want_V=False)
        t1 = time.perf_counter()
        cert = sdr.certify_batch(C, o['y'], o['sweeps'], 5000)
        t2 = time.perf_counter()
        return t2 - t0, t1 - t0, o, cert

    batched()                                       # warm-up: code object, buffers
    runs = sorted((batched() for _ in range(args.repeat)), key=lambda r: r[0])
    t_batched, t_call, o, cert = runs[len(runs) // 2]

    nl = min(args.loop_problems, args.B)

    def loop():
        out = []
        t0 = time.perf_counter()
        for b in range(nl):
            q = QCQP(Problem.from_minimize_form(fl[b]))
            q.suggest(s.SDR, num_samples=args.S, seed=args.seed + b)
            out.append((q.sdr_bound, bool(q.sdr_info.get('converged')), int(q.sdr_info.get('sweeps', -1))))
            q.engine.close()
        return time.perf_counter() - t0, out

    loop()                                          # warm-up
    t_loop, single = sorted((loop() for _ in range(3)), key=lambda t: t[0])[1]
    both = [b for b in range(nl) if single[b][1] and single[b][0] is not None and cert['converged'][b]]
    diff = max([abs(single[b][0] - cert['bound'][b]) / (1.0 + abs(single[b][0])) for b in both] or [float('nan')])
    print(json.dumps(dict(
        workload=dict(B=args.B, n=args.n, m=args.m, S=args.S, max_sweeps=5000, tol=1e-11), kernel='sdr_small_kernel<true>' if args.wide and args.n > 64 else 'sdr_small_kernel',
        batched_s=t_batched, batched_call_s=t_call, batched_certify_s=t_batched - t_call, batched_all_s=[r[0] for r in runs],
        certified='%d/%d' % (int(cert['converged'].sum()), args.B), sweeps_mean=float(np.mean(o['sweeps'])), sweeps_max=int(np.max(o['sweeps'])),
        loop_problems=nl, loop_s_measured=t_loop, loop_s_scaled_to_B=t_loop * args.B / nl, loop_scaling='linear in B (not measured beyond loop_problems)',
        speedup=(t_loop * args.B / nl) / t_batched, both_certified='%d/%d' % (len(both), nl), max_rel_bound_difference=diff,
        loop_sweeps_mean=float(np.mean([x[2] for x in single])))))


if __name__ == '__main__':
    main()
