"""The rules, masks and clouds the grade tests share (tests/test_grade.py on the host, tests/test_grade_gpu.py on the GPU)."""
import numpy as np

import transform_cases as TC

N = TC.N                               # 357: five full clusters of 64 and one of 37
masks, selected = TC.masks, TC.selected
W709 = np.array([0.2126, 0.7152, 0.0722])
GRADE_COLOUR, GRADE_ALPHA = 1, 2

# name -> keyword arguments of engine.grade_params (the rule is grade_prepare's), or a matrix for engine.grade_rule
PARAMS = {
    "exposure +1": dict(exposure=1.0),                                   # M = 2 I: exact in halves away from overflow
    "exposure -1": dict(exposure=-1.0),
    "tint": dict(gain=(1.2, 0.9, 0.7)),
    "grey": dict(saturation=0.0),
    "sat_1_5": dict(saturation=1.5),
    "contrast": dict(contrast=1.3, pivot=0.5),
    "lift": dict(offset=(0.05, 0.02, -0.03)),
    "alpha_half": dict(alpha_gain=0.5),
    "alpha_lift": dict(alpha_gain=1.0, alpha_offset=0.3),                 # reaches the clamp at 1
    "all": dict(exposure=0.4, gain=(1.1, 0.95, 0.8), saturation=1.3, contrast=1.2, pivot=0.45, offset=(0.03, -0.02, 0.01),
                alpha_gain=0.8, alpha_offset=0.05),
    "neutral": dict(),
}
MATRICES = {"channel_swap": [[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0]]}     # red <-> blue: a permutation, exact, its own inverse
RULES = tuple(PARAMS) + tuple(MATRICES)
# which steps each rule runs
FLAGS = {name: GRADE_COLOUR for name in RULES}
FLAGS.update({"alpha_half": GRADE_ALPHA, "alpha_lift": GRADE_ALPHA, "all": GRADE_COLOUR | GRADE_ALPHA, "neutral": 0})


def make_rule(pkg, name):
    """the rule dict (engine.grade_prepare / engine.grade_rule) of a named case"""
    E = pkg.engine
    if name in MATRICES:
        return E.grade_rule(MATRICES[name])
    return E.grade_prepare(E.grade_params(**PARAMS[name]))


def cloud(pkg, sh=True, n=N, seed=11):
    """finite data; splats large enough to overlap on the GPU tests' 96 x 64 frames (test_move_gpu._cloud's arguments)"""
    return pkg.scenes.make_scene(n, seed=seed, sh=sh, log_scale_range=(-3.5, -2.0))


def compose64(exposure=0.0, gain=(1.0, 1.0, 1.0), saturation=1.0, contrast=1.0, pivot=0.5, offset=(0.0, 0.0, 0.0), alpha_gain=1.0,
              alpha_offset=0.0):
    """(M, b) in float64 of the three steps, composed as matrices from the float32 values of the parameters -- written apart from the
    library's closed form: c1 = 2^e gain o c;  c2 = L + s (c1 - L), L = w . c1;  c3 = k (c2 - pivot) + pivot + offset"""
    f = lambda v: np.asarray(v, np.float32).astype(np.float64)
    S1 = np.diag(2.0 ** float(f(exposure)) * f(gain))
    S2 = float(f(saturation)) * np.eye(3) + (1.0 - float(f(saturation))) * np.outer(np.ones(3), W709)
    k, p = float(f(contrast)), float(f(pivot))
    return k * (S2 @ S1), p - k * p + f(offset)
