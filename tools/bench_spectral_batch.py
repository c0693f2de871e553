"""Wall time of the batched spectral suggest (qcqpmi_spectral_small_batch) against the host doing the same work and against the
per-problem solver it replaces.

Workload: problems.boolean_least_squares_batch(B, n, m); the launch at its defaults (max_sweeps = 30, tol = 1e-15).
  batched    ONE call of Engine.spectral_small_batch (uploads of the B objectives, the launch, the downloads of x, bound, mu, lam,
             sweeps, branch, status): host clock around it, --repeat calls after one warm-up; median and spread.
  host       the same work on the host: ONE batched numpy.linalg.eigh of the B matrices A_b, then the independent secular solver of
             tests/spectral_batch_cases.py problem by problem (a bracketed root); eigh's share is reported on its own.  BLAS pools as
             the process finds them.
  loop       what the library offered before: sdr.solve_spectral per problem (an auxiliary context, the general Burer-Monteiro /
             augmented-Lagrangian solver, eigh of X).  Timed on the first --loop-problems problems and SCALED LINEARLY to B (every
             problem costs the same work; stated as such in the output).
--wide: the same three columns for 65 <= n <= 128 through Engine.spectral_batch (qcqpmi_spectral_batch, spectral_wide_kernel); the
defaults become B = 1024, n = 128, m = 192.
Prints one JSON line (with the sweeps per problem, the branches taken and the largest relative difference of the bounds).
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--wide', action='store_true', help='qcqpmi_spectral_batch (n <= 128); defaults B = 1024, n = 128, m = 192')
    ap.add_argument('--B', type=int, default=None)
    ap.add_argument('--n', type=int, default=None)
    ap.add_argument('--m', type=int, default=None)
    ap.add_argument('--repeat', type=int, default=5)
    ap.add_argument('--loop-problems', type=int, default=16)
    ap.add_argument('--seed', type=int, default=1)
    args = ap.parse_args()
    for key, narrow, wide in (('B', 4096, 1024), ('n', 32, 128), ('m', 48, 192)):
        if getattr(args, key) is None:
            setattr(args, key, wide if args.wide else narrow)

    import numpy as np
    import spectral_batch_cases as sc
    from qcqp_amd import problems, sdr
    from qcqp_amd.batch import QCQPBatch
    from qcqp_amd.engine import device_count
    from qcqp_amd.form import QCQPForm
    if device_count() < 1:
        raise SystemExit('bench_spectral_batch: no HIP device visible (there is no CPU path)')

    fl = problems.boolean_least_squares_batch(args.B, args.n, args.m, seed=args.seed)
    qb = QCQPBatch(fl)
    agg, relop = qb._spectral_aggregate()
    launch = qb.engine.spectral_batch if args.wide else qb.engine.spectral_small_batch

    def batched():
        t0 = time.perf_counter()
        o = launch(qb.P0s, qb.q0s, qb.r0s, agg, relop)
        return time.perf_counter() - t0, o

    batched()                                       # warm-up: code object, buffers
    runs = sorted((batched() for _ in range(args.repeat)), key=lambda r: r[0])
    t_batched, o = runs[len(runs) // 2]
    print('batched: %.4f s' % t_batched, file=sys.stderr, flush=True)

    def host():
        t0 = time.perf_counter()
        s = np.sqrt(agg[:args.n])
        lam, Q = np.linalg.eigh(qb.P0s / np.outer(s, s))
        t1 = time.perf_counter()
        bound = np.array([sc.independent(qb.P0s[b], qb.q0s[b], qb.r0s[b], agg, relop, eig=(lam[b], Q[b]))['bound'] for b in range(args.B)])
        return time.perf_counter() - t0, t1 - t0, bound

    host()
    hruns = sorted((host() for _ in range(args.repeat)), key=lambda r: r[0])
    t_host, t_eigh, hbound = hruns[len(hruns) // 2]
    print('host: %.4f s (eigh %.4f s)' % (t_host, t_eigh), file=sys.stderr, flush=True)

    nl = min(args.loop_problems, args.B)

    def loop(count):
        t0 = time.perf_counter()
        vals = [sdr.solve_spectral(QCQPForm.from_arrays(fl[b]))[1] for b in range(count)]
        return time.perf_counter() - t0, vals

    print('loop warm-up: %.2f s for one problem' % loop(1)[0], file=sys.stderr, flush=True)      # the code objects of the dense path
    t_loop, single = loop(nl)
    rel = lambda a, b: float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / (1.0 + np.abs(np.asarray(b)))))
    print(json.dumps(dict(
        workload=dict(B=args.B, n=args.n, m=args.m, max_sweeps=30, tol=1e-15), kernel='spectral_wide_kernel' if args.wide and args.n > 64 else 'spectral_small_kernel',
        batched_s=t_batched, batched_all_s=[r[0] for r in runs], host_s=t_host, host_eigh_s=t_eigh, host_all_s=[r[0] for r in hruns],
        speedup_over_host=t_host / t_batched, speedup_over_host_eigh_alone=t_eigh / t_batched,
        status_ok='%d/%d' % (int(np.sum(o['status'] == 0)), args.B), sweeps_mean=float(np.mean(o['sweeps'])), sweeps_max=int(np.max(o['sweeps'])),
        branches=[int(np.sum(o['branch'] == k)) for k in range(3)], max_rel_bound_difference_host=rel(o['bound'], hbound),
        loop_problems=nl, loop_s_measured=t_loop, loop_s_scaled_to_B=t_loop * args.B / nl, loop_scaling='linear in B (not measured beyond loop_problems)',
        speedup_over_loop_scaled=(t_loop * args.B / nl) / t_batched, max_rel_gap_loop=rel(single, o['bound'][:nl]))))
    qb.close()


if __name__ == '__main__':
    main()
