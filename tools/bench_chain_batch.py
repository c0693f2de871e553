"""Wall time of an improve chain on QCQPBatch: ONE launch of the chain kernel (qcqpmi_chain_small_batch_run) against the COMPOSED path
-- the single engine calls stage by stage, X of one as X0 of the next -- on the SAME build.

Workload: problems.boolean_least_squares_batch(B, n, m), R restarts per problem, the chain [ADMM(num_iters), COORD_DESCENT(cd_iters)]
(the reference's improve(ADMM); improve(COORD_DESCENT) of its examples).  Default shapes: B = 4096, n = 32 and B = 1024, n = 64, R = 64.
  fused      QCQPBatch.improve([ADMM, CD], fused=None)
  composed   QCQPBatch.improve([ADMM, CD], fused=False): two launches with a download and an upload of B R n doubles and a device-wide
             join between them
  singles    improve(ADMM) + improve(COORD_DESCENT), each from suggest()'s points: NOT the same computation (coordinate descent starts
             from the normals, not from ADMM's points); the sum is reported for orientation only
Every call computes rho and the inverses on the host (one batched eigvalsh, one batched inverse: setup='host'), which is timed on its
own and is the same in the paths compared.  Host clock around improve(), which ends synchronised.  After one warm-up of every path
the paths ALTERNATE --repeat times (fused, composed, singles, fused, ...); the medians and every single time are printed, one JSON line
per shape.  The line also says whether fused and composed agree bit for bit on the winners at the timed size."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def median(v):
    return sorted(v)[len(v) // 2]


def shape(B, n, R, args):
    import numpy as np
    from qcqp_amd import batch, problems, settings as s
    from qcqp_amd.batch import QCQPBatch
    fl = problems.boolean_least_squares_batch(B, n, n + n // 2, seed=args.seed)
    qb = QCQPBatch(fl)
    qb.suggest(s.RANDOM, num_samples=R, seed=args.seed)
    chain = [(s.ADMM, dict(num_iters=args.num_iters)), (s.COORD_DESCENT, dict(num_iters=args.cd_iters))]

    def timed(fn):
        t0 = time.perf_counter()
        out = fn()
        return time.perf_counter() - t0, out

    def fused():
        f, _ = qb.improve(chain, fused=None)
        return f, qb.x, qb.last_stats['kernel']

    def composed():
        f, _ = qb.improve(chain, fused=False)
        return f, qb.x, qb.last_stats['kernel']

    def singles():
        qb.improve(s.ADMM, num_iters=args.num_iters)
        f, _ = qb.improve(s.COORD_DESCENT, num_iters=args.cd_iters)
        return f, qb.x, None

    paths = (('fused', fused), ('composed', composed), ('singles', singles))
    last = {}
    for name, fn in paths:                          # warm-up: code objects, buffers
        last[name] = fn()
    times = dict((name, []) for name, _ in paths)
    for _ in range(args.repeat):
        for name, fn in paths:
            t, last[name] = timed(fn)
            times[name].append(t)
    t_host, _ = timed(lambda: batch.admm_minvs(qb.P0s, batch.admm_rhos(qb.P0s, qb.form.m), qb.form.m))
    same = bool(np.array_equal(last['fused'][0], last['composed'][0]) and np.array_equal(last['fused'][1], last['composed'][1]))
    out = dict(workload=dict(family='bls', B=B, n=n, m=n + n // 2, R=R, chain='ADMM(%d) + CD(%d)' % (args.num_iters, args.cd_iters)),
               kernel_fused=last['fused'][2], kernel_composed=last['composed'][2], fused_s=median(times['fused']),
               composed_s=median(times['composed']), singles_sum_s=median(times['singles']), composed_over_fused=median(times['composed']) / median(times['fused']),
               fused_all_s=times['fused'], composed_all_s=times['composed'], singles_all_s=times['singles'],
               host_eigvalsh_and_inverse_s=t_host, transfer_doubles_each_way=B * R * n, winners_bit_for_bit=same)
    qb.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='4096x32x64,1024x64x64', help='B x n x R, comma separated')
    ap.add_argument('--num-iters', type=int, default=100, help='ADMM iterations per phase')
    ap.add_argument('--cd-iters', type=int, default=1000)
    ap.add_argument('--repeat', type=int, default=5)
    ap.add_argument('--seed', type=int, default=1)
    args = ap.parse_args()
    from qcqp_amd.engine import device_count
    if device_count() < 1:
        raise SystemExit('bench_chain_batch: no HIP device visible (there is no CPU path)')
    for sh in args.shapes.split(','):
        B, n, R = (int(v) for v in sh.split('x'))
        shape(B, n, R, args)


if __name__ == '__main__':
    main()
