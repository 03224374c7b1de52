"""The yardstick of the float32 step parity (tests/test_gpu_f32_step_parity.py), pinned on the CPU: how far an honest
float32 implementation of the tick, in the reference's operation order, is from the f64 oracle on float32-rounded inputs.
The GPU gate is 4 x this restatement's error (floor 8 * 2^-24); the cap asserted here keeps that gate below
128 * 2^-24 = 7.6e-6 whatever inputs a later edit picks."""
import numpy as np
import pytest

from tests import f32_parity_util as fu
from tests import parity

N = 130
NAMES = {fu.L.RK4: "rk4", fu.L.SEMI_IMPLICIT: "semi_implicit"}


def test_f64_instantiation_of_the_restatement_equals_the_c_oracle():
    """The same numpy code in float64 is the oracle's arithmetic: bit for bit on every pipe of the matrix, both integrators
    (a mistake in `builtin_effectors` would otherwise bend the yardstick, not fail a test)."""
    cols = {k: v[:N] for k, v in fu.world().items()}
    for name, pipe in fu.PIPES.items():
        for integrator in fu.INTEGRATORS:
            want = fu.run_oracle(pipe, integrator, cols)
            got = fu.run_restatement(pipe, integrator, cols, dtype=np.float64)
            for t in fu.TICKS:
                for f in parity.FIELDS:
                    assert np.array_equal(getattr(got[t], f), getattr(want[t], f)), (name, integrator, t, f)


def test_float32_restatement_stays_within_32_ulp_of_the_oracle():
    lines, worst = [], {}
    for name in fu.PIPES:
        for integrator in fu.INTEGRATORS:
            ref, rest = fu.references(name, integrator)
            for t in fu.TICKS:
                errs = fu.half_errors(fu.rows_of(rest[t], slice(0, N)), fu.rows_of(ref[t], slice(0, N)))
                whole = parity.state_errors(fu.rows_of(rest[t], slice(0, N)), fu.rows_of(ref[t], slice(0, N)))
                assert all(whole[f] == max(errs[f + ".a"], errs[f + ".b"]) for f in parity.FIELDS)
                worst[(name, integrator, t)] = errs
                lines.append(f"restatement {name:28s} {NAMES[integrator]:13s} n {N} ticks {t}: {fu.fmt(errs)}  [2^-24]")
    fu.record(lines, "f32_restatement_host.txt")
    top = max(worst, key=lambda k: max(worst[k].values()))
    print("worst:", top, max(worst[top].values()) / fu.U32, "x 2^-24")
    for key, errs in worst.items():
        for half, v in errs.items():
            assert v <= fu.RESTATEMENT_CAP, (key, half, v / fu.U32)
    assert max(worst[top].values()) > 0.5 * fu.U32, "a float32 run that is exact against f64 did not run in float32"


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_restatement_keeps_the_dtype_of_its_state(dtype):
    cols = {k: v[:5] for k, v in fu.world().items()}
    out = fu.run_restatement(fu.PIPES["interp_four_aux"], fu.L.RK4, cols, dtype=dtype)    # asserts the dtype of every tick inside
    assert np.isfinite(out[4].world_pos).all()
