"""Wall time of the small-problem batch (qcqpmi_cd_small_batch_run) against the per-problem loop it replaces.

Workload: problems.boolean_least_squares_batch(B, n, m), R restarts per problem, num_iters sweeps at most.
  batched    ONE call of Engine.cd_small_batch_run (uploads of the B objectives, the launch, the downloads of the per-restart
             results and the winners): host clock around the call, which ends synchronised; --repeat calls after one warm-up, median.
  loop       what the library offered before for the same restarts: per problem a fresh context (set_quad of the constraints and
             objective b, finalize -- a context cannot take a second objective after finalize --), randn, cd_run, select_best.
             Timed on the first --loop-problems problems and SCALED LINEARLY to B (every problem costs the same launches).
Prints one JSON line (with how many winners of the timed subset the two paths agree on).  --profile-run: only the batched call, once
after a warm-up (for rocprofv3 --kernel-trace --stats).

--per-problem-constraints: the workload is problems.per_problem_constraints_batch('boxpp', n, seeds) -- box-constrained indefinite QPs
with bounds per instance -- and the batched call is qcqpmi_cd_small_batch_run_pc (Engine.cd_small_batch_run(cons=...)).  The loop is the
best the library offered for such a batch before: per problem a fresh context from the problem's own functions and ONE call of
qcqpmi_cd_small_batch_run with B = 1 (bit for bit the same restarts), timed on --loop-problems problems and scaled linearly to B.

--n above 64 (up to 128): the batched call is qcqpmi_cd_batch_run (Engine.cd_batch_run, the wide kernels: two coordinates per lane), e.g.
--n 128 --m 192 --B 1024 --loop-problems 64 for a frame of 64 x 64 QPSK MIMO detection problems; the loop is the same as for n <= 64.
--wide-threads T: the wide kernels' workgroup size for this run (QCQPMI_CD_WIDE_THREADS; the library's choice is 512).
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
    ap.add_argument('--R', type=int, default=64)
    ap.add_argument('--num-iters', type=int, default=1000)
    ap.add_argument('--repeat', type=int, default=5)
    ap.add_argument('--loop-problems', type=int, default=256)
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--profile-run', action='store_true')
    ap.add_argument('--per-problem-constraints', action='store_true')
    ap.add_argument('--wide-threads', type=int, default=0)
    args = ap.parse_args()
    if args.wide_threads:
        os.environ['QCQPMI_CD_WIDE_THREADS'] = str(args.wide_threads)      # read once, by the first wide launch

    from qcqp_amd import problems
    from qcqp_amd.batch import QCQPBatch
    from qcqp_amd.engine import Engine, device_count
    from qcqp_amd.form import QCQPForm
    if device_count() < 1:
        raise SystemExit('bench_small_batch: no HIP device visible (there is no CPU path)')

    pc = args.per_problem_constraints
    if pc:
        fl = problems.per_problem_constraints_batch('boxpp', args.n, [args.seed + b for b in range(args.B)])
    else:
        fl = problems.boolean_least_squares_batch(args.B, args.n, args.m, seed=args.seed)
    qb = QCQPBatch(fl)
    e = qb.engine
    kw = dict(cons=qb.cons) if pc else {}

    run = e.cd_small_batch_run if args.n <= 64 else e.cd_batch_run

    def batched():
        t0 = time.perf_counter()
        o = run(qb.P0s, qb.q0s, qb.r0s, args.R, num_iters=args.num_iters, seed=args.seed, seed_stride=1, want_x=False, **kw)
        return time.perf_counter() - t0, o

    batched()                                       # warm-up: code object, buffers
    if args.profile_run:
        t, o = batched()
        print(json.dumps(dict(mode='profile-run', batched_s=t, kernel=e.last_cd_kernel())))
        return
    runs = [batched() for _ in range(args.repeat)]
    times = sorted(t for t, _ in runs)
    o = runs[-1][1]
    t_batched = times[len(times) // 2]
    kernel_ms = e.kernel_ms(Engine.KERNEL_CD2)
    sweeps = int(o['sweeps1'].sum() + o['sweeps2'].sum())

    nl = min(args.loop_problems, args.B)

    def loop():
        best = []
        t0 = time.perf_counter()
        for b in range(nl):
            eb = Engine(QCQPForm.from_arrays(fl[b]))
            if pc:
                ob = (eb.cd_small_batch_run if args.n <= 64 else eb.cd_batch_run)(qb.P0s[b:b + 1], qb.q0s[b:b + 1], qb.r0s[b:b + 1], args.R,
                                                                                  num_iters=args.num_iters, seed=args.seed + b, want_x=False)
                best.append((int(ob['best_index'][0]), float(ob['best_f0'][0])))
            else:
                eb.randn(args.R, seed=args.seed + b)
                eb.cd_run(num_iters=args.num_iters, seed=args.seed + b)
                best.append(eb.select_best())
            eb.close()
        return time.perf_counter() - t0, best

    loop()                                          # warm-up
    lt = sorted((loop() for _ in range(3)), key=lambda t: t[0])
    t_loop, best = lt[1]
    agree = sum(1 for b in range(nl) if int(o['best_index'][b]) == best[b][0] and abs(o['best_f0'][b] - best[b][1]) <= 1e-9 * (1 + abs(best[b][1])))
    print(json.dumps(dict(
        workload=dict(family='boxpp' if pc else 'bls', B=args.B, n=args.n, m=args.m, R=args.R, num_iters=args.num_iters), kernel=e.last_cd_kernel(),
        wide_threads=args.wide_threads or None,
        batched_s=t_batched, batched_all_s=times, batched_kernel_ms=kernel_ms, restart_sweeps=sweeps,
        restart_sweeps_per_s=sweeps / t_batched, loop_problems=nl, loop_s_measured=t_loop,
        loop_s_scaled_to_B=t_loop * args.B / nl, speedup=(t_loop * args.B / nl) / t_batched, winners_agree='%d/%d' % (agree, nl))))


if __name__ == '__main__':
    main()
