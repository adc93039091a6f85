"""Continuation in the regulariser's weight (reference:
python/continuation_solver.py:2-11): eleven warm-started solves at lambda = 0,
0.1, .., 1, each from the last one's solution.

`solve` keeps the reference's signature over caller closures f(x, lamb) and
nabla_f(x, lamb).  `solve_engine` is the same ramp on the fused device engine:
set_regulariser(lam * i / steps) between warm-started BBEngine.solve calls, on
one set of images.
"""
import BB

STEPS = 10


def solve(x0, f, nabla_f, stopping, record_every=500, proj=None, log=None, options=None,
          solve=BB.solve):
    x = x0
    for lamb in (i / float(STEPS) for i in range(STEPS + 1)):
        x = solve(x, lambda v, l=lamb: f(v, l), lambda v, l=lamb: nabla_f(v, l), stopping,
                  record_every=record_every, proj=proj, log=log, options=options)
    return x


def solve_engine(eng, z0, lam, steps=STEPS, record_every=500, log=None, poll=50):
    """The ramp on a device.BBEngine: lambda = lam * i / steps for i = 0 ..
    steps (the engine's reg_weights kept), each solve started from the last
    one's z.  Returns the final z (a device tensor); the engine is left at
    lambda = lam."""
    from device import reg_lambda_check
    lam = reg_lambda_check(lam)
    if isinstance(steps, bool) or int(steps) != steps or steps < 1:
        raise ValueError('steps must be an int >= 1 (got %r)' % (steps,))
    z = z0
    for i in range(int(steps) + 1):
        eng.set_regulariser(lam * i / float(steps))
        z = eng.solve(z0=z, log=log, record_every=record_every, poll=poll).clone()
    return z
