"""Vectorised numpy restatement of the six_dof tick with a pluggable effector callback, in the reference's
operation order (same citations as oracle/sixdof_oracle.c; numpy has no FMA contraction).  Used where the
effectors are user-written (elodin_amd.dsl) and the C oracle's built-in set does not apply.  It is itself
checked bit-for-bit against the C oracle on built-in effectors (tests/test_dsl_host.py).  Dtype-preserving: every
constant and every zero takes the dtype of the state, so float32 columns give the tick in float32 arithmetic (the
yardstick of tests/test_f32_restatement_host.py).  TEST INFRASTRUCTURE."""
import numpy as np


def qmul(l, r):  # quaternion.rs:268-281
    li, lj, lk, lw = l.T
    ri, rj, rk, rw = r.T
    return np.stack([lw * ri + li * rw + lj * rk - lk * rj, lw * rj - li * rk + lj * rw + lk * ri,
                     lw * rk + li * rj - lj * ri + lk * rw, lw * rw - li * ri - lj * rj - lk * rk], axis=1)


def dot(a, b):
    acc = a[:, 0] * b[:, 0]
    for k in range(1, a.shape[1]):
        acc = acc + a[:, k] * b[:, k]
    return acc


def qinv(q):  # quaternion.rs:141-155
    d = dot(q, q)[:, None]
    return np.concatenate([-q[:, :3], q[:, 3:]], axis=1) / d


def rot(q, v):  # quaternion.rs:283-305
    vq = np.concatenate([v, np.zeros((len(v), 1), dtype=v.dtype)], axis=1)
    return qmul(qmul(q, vq), qinv(q))[:, :3]


def add_motion(x, m):  # spatial.rs:530-549
    ho = np.concatenate([m[:, :3] / m.dtype.type(2.0), np.zeros((len(m), 1), dtype=m.dtype)], axis=1)
    s = x[:, :4] + qmul(ho, x[:, :4])
    s = s / np.sqrt(dot(s, s))[:, None]
    return np.concatenate([s, x[:, 4:] + m[:, 3:]], axis=1)


def calc_accel(F, I, x):  # six_dof.rs:137-146
    q = x[:, :4]
    qi = qinv(q)
    bt, bf = rot(qi, F[:, :3]), rot(qi, F[:, 3:])
    return np.concatenate([rot(q, bt / I[:, :3]), rot(q, bf / I[:, 6:7])], axis=1)


def tick(pos, vel, accel, inertia, effectors, dt_g, dt=None, integrator=0):
    """One tick; effectors(xs, vs) -> F [n,6].  Returns pos, vel, accel, force."""
    T = pos.dtype.type
    dt_g, dt = T(dt_g), T(dt_g if dt is None else dt)
    if integrator == 1:  # semi_implicit.rs:17-62
        F = effectors(pos, vel)
        A = calc_accel(F, inertia, pos)
        vel = vel + dt * A
        return add_motion(pos, dt * vel), vel, A, F
    A_prev, V, A = accel, [], []
    for c in (T(0.0), T(0.5), T(0.5), T(1.0)):  # rk4.rs:87-135
        h = dt_g * c
        xs = add_motion(pos, h * vel)
        vs = vel + h * A_prev
        F = effectors(xs, vs)
        A_prev = calc_accel(F, inertia, xs)
        V.append(vs)
        A.append(A_prev)
    g = dt * T(1.0 / 6.0)
    sv = g * (V[0] + T(2.0) * V[1] + T(2.0) * V[2] + V[3])
    sa = g * (A[0] + T(2.0) * A[1] + T(2.0) * A[2] + A[3])
    return add_motion(pos, sv), vel + sa, A[3], F
