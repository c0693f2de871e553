"""Wall time of the batched ADMM (qcqpmi_admm_small_batch_run; --wide: qcqpmi_admm_batch_run, n <= 128) against the per-problem loop it
replaces.

Workload: problems.boolean_least_squares_batch(B, n, m), R restarts per problem, num_iters iterations per phase at most.
  batched    QCQPBatch.suggest(RANDOM) + improve(ADMM): one batched eigvalsh (the rho rule), one batched inverse, ONE launch of
             admm_small_kernel, the downloads of the per-restart results and the winners.  Host clock around improve(), which ends
             synchronised; --repeat calls after one warm-up, median.  The host part (eigvalsh + inverse) is timed on its own as well.
  loop       what the library offered before: per problem QCQP(Problem).suggest(RANDOM, R) + improve(ADMM) -- a context, finalize,
             a Lanczos run for lambda_min, the inverse, several launches per iteration.  Timed on the first --loop-problems problems and
             SCALED LINEARLY to B (every problem costs the same launches).  --loop-problems 0 skips it (an A/B of the batched call alone).
--wide passes wide=True to improve(ADMM), so that --n 128 --m 192 runs (the wide kernels); --wide-threads T sets
QCQPMI_ADMM_WIDE_THREADS: a workgroup of T threads for the wide kernels instead of the occupancy rule (results do not depend on it).
--setup device passes setup='device' to improve(ADMM): rho and the inverses come from one launch of the setup kernels
(qcqpmi_admm_batch_setup) instead of the batched eigvalsh and inverse; that call alone (upload of the B objectives,
the launch, the downloads of the B inverses) is then timed as well, next to the host part.  The default, host, is the path every
earlier figure of this tool was taken on.
Prints one JSON line.  The two paths agree in the median only (the iteration amplifies rounding: DESIGN.md 4.13); the line reports on how
many of the timed problems the winners' objectives agree to 1e-6."""
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
    ap.add_argument('--R', type=int, default=64)
    ap.add_argument('--num-iters', type=int, default=100)
    ap.add_argument('--repeat', type=int, default=5)
    ap.add_argument('--loop-problems', type=int, default=64)
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--wide', action='store_true')
    ap.add_argument('--wide-threads', type=int, default=0)
    ap.add_argument('--setup', choices=('host', 'device'), default='host')
    args = ap.parse_args()
    if args.wide_threads:
        os.environ['QCQPMI_ADMM_WIDE_THREADS'] = str(args.wide_threads)      # read once, at the first wide launch

    from qcqp_amd import QCQP, Problem, batch, problems, settings as s
    from qcqp_amd.batch import QCQPBatch
    from qcqp_amd.engine import device_count
    if device_count() < 1:
        raise SystemExit('bench_admm_batch: no HIP device visible (there is no CPU path)')

    fl = problems.boolean_least_squares_batch(args.B, args.n, args.m, seed=args.seed)
    qb = QCQPBatch(fl)
    qb.suggest(s.RANDOM, num_samples=args.R, seed=args.seed)

    kw = dict(wide=True) if args.wide else {}
    if args.setup != 'host':                        # (the default call carries no keyword: the path of the earlier figures)
        kw['setup'] = args.setup

    def batched():
        t0 = time.perf_counter()
        f, v = qb.improve(s.ADMM, num_iters=args.num_iters, **kw)
        return time.perf_counter() - t0, f

    batched()                                       # warm-up: code object, buffers
    runs = [batched() for _ in range(args.repeat)]
    times = sorted(t for t, _ in runs)
    f_batched = runs[-1][1]
    t_batched = times[len(times) // 2]
    t0 = time.perf_counter()
    rhos = batch.admm_rhos(qb.P0s, qb.form.m)
    batch.admm_minvs(qb.P0s, rhos, qb.form.m)
    t_host = time.perf_counter() - t0
    st = qb.last_stats
    t_dev = None
    if args.setup == 'device':
        dev = []
        for _ in range(args.repeat + 1):            # the first call is the warm-up
            t0 = time.perf_counter()
            qb.engine.admm_batch_setup(qb.P0s)
            dev.append(time.perf_counter() - t0)
        t_dev = sorted(dev[1:])[len(dev[1:]) // 2]
    iters = int(st['iters1'].sum() + st['iters2'].sum())

    nl = min(args.loop_problems, args.B)

    def loop():
        best = []
        t0 = time.perf_counter()
        for b in range(nl):
            q = QCQP(Problem.from_minimize_form(fl[b]))
            q.suggest(s.RANDOM, num_samples=args.R, seed=args.seed + b)
            fb, vb = q.improve(s.ADMM, num_iters=args.num_iters)
            best.append(float(fb))
        return time.perf_counter() - t0, best

    out = dict(workload=dict(family='bls', B=args.B, n=args.n, m=args.m, R=args.R, num_iters=args.num_iters), kernel=st['kernel'],
               wide_threads=args.wide_threads or 'rule', batched_s=t_batched, batched_all_s=times, setup=args.setup, host_eigvalsh_and_inverse_s=t_host, device_setup_call_s=t_dev,
               restart_iterations=iters, restart_iterations_per_s=iters / t_batched, loop_problems=nl)
    if nl > 0:
        loop()                                      # warm-up
        lt = sorted((loop() for _ in range(3)), key=lambda t: t[0])
        t_loop, best = lt[1]
        agree = sum(1 for b in range(nl) if abs(f_batched[b] - best[b]) <= 1e-6 * (1 + abs(best[b])))
        out.update(loop_s_measured=t_loop, loop_s_scaled_to_B=t_loop * args.B / nl, speedup_scaled=(t_loop * args.B / nl) / t_batched,
                   winners_objective_agree_1e6='%d/%d' % (agree, nl))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
