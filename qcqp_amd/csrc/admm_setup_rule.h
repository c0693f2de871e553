// The two scalar pieces of the device-side ADMM setup (admm_setup.h), written so that a host program can test them
// (tests/host/admm_setup_selftest.cpp): the reference's rho rule and the weight of an eigen-direction in the inverse.
// Both in the order of operations of their host counterparts (qcqp_amd/batch.py: admm_rhos, admm_minvs; the build has
// -ffp-contract=off), so equal inputs give equal bits.
#pragma once
#include <hip/hip_runtime.h>

namespace qcqpmi {

// improve_admm's rule (qcqp.py:270-277) from lambda_min(P0) and the number of constraints m:
// 50 * 2 (1 - lambda_min) / m where lambda_min < 0, else 50 / m.  A NaN takes the second branch, as numpy.where does.
__host__ __device__ inline double admm_setup_rho(double lmin, double m) {
    return lmin < 0.0 ? 50.0 * ((2.0 * (1.0 - lmin)) / m) : 50.0 * (1.0 / m);
}

// whether a GIVEN rho is too small for the problem (the reference's test: lambda_min + m rho < 0)
__host__ __device__ inline bool admm_setup_rho_too_small(double lmin, double m, double rho) { return lmin + m * rho < 0.0; }

// 1 / (2 (lam + rho m)): the eigenvalue of (2 (P0 + rho m I))^-1 on the eigenvector of lam
__host__ __device__ inline double admm_setup_weight(double lam, double rho, double m) { return 1.0 / (2.0 * (lam + rho * m)); }

}  // namespace qcqpmi
