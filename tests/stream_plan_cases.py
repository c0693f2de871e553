"""The shapes tests/test_gpu_stream_plan.py runs, and the kernel the plan gives each of them: rows of the table of
tests/host/stream_plan_selftest.cpp (tests/test_stream_plan_cpu.py checks that each name stands there)."""

# (shape, switches) -> kernel name, as the selftest's table asserts them (each line below is a CHECK of that file)
KERNEL_NAMES = {
    ('bls48', 'default'): 'cd_life_kernel<3,band>',
    ('bls40', 'default'): 'cd_life_kernel<3,band>',
    ('bls128_rank16', 'default'): 'cd_life_kernel<3,band,factored>',
    ('bls128_rank16', 'life_version3'): 'cd_life_kernel<3,band>',
    ('bls48', 'life_version1'): 'cd_phase2_qs_kernel<lifecycle>',
    ('maxcut64', 'default'): 'cd_life_kernel<3,lin>',
}
