"""The staged forms of the table-driven exp in colate_amd/csrc/em_math.hpp (em_exp_tab_k / _r / _poly / _value / _value_om, which the
hand-scheduled EM loop issues with another chain's instructions in between) give the doubles of em_exp_t / em_exp_om_t: the same
operations on the same operands, checked on the host build of the header, bit for bit.  The device build of the stages -- and the
staged reciprocal, which on the host is the plain division either way -- is covered by the byte equality across the builds in
tests/test_gpu_role_a_front.py, not here."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
dp = ctypes.POINTER(ctypes.c_double)

SRC = r'''
#include "%s/colate_amd/csrc/em_math.hpp"
static double staged(double x, bool neg, double* om) {
  const double xc = neg ? em::max_c_neg(x, -1100.0) : em::max_c(x, -1100.0);
  const em::ExpK k = em::em_exp_tab_k(xc);
  const int ki = em::em_lo32(k.kd), e = ki >> 5, j = 2 * (ki & 31);
  const double r = em::em_exp_tab_r(xc, k.k);
  const double th = em::kExpTableHost[j], tl = em::kExpTableHost[j + 1];
  const double p = em::em_exp_tab_poly(r);
  return om ? em::em_exp_tab_value_om(th, tl, p, e, om) : em::em_exp_tab_value(th, tl, p, e);
}
extern "C" {
void whole(int n, const double* x, double* y, double* z, double* w) {
  for (int i = 0; i < n; i++) { y[i] = em::em_exp_t(x[i], em::kExpTableHost); z[i] = em::em_exp_om_t<true>(-x[i], &w[i], em::kExpTableHost); }
}
void stages(int n, const double* x, double* y, double* z, double* w) {
  for (int i = 0; i < n; i++) { y[i] = staged(x[i], false, nullptr); z[i] = staged(-x[i], true, &w[i]); }
}
}
'''


@pytest.fixture(scope="module")
def m(tmp_path_factory):
    d = tmp_path_factory.mktemp("emmath_stages")
    src = d / "h.cpp"
    src.write_text(SRC % ROOT)
    so = d / "libh.so"
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", str(so), str(src)])
    return ctypes.CDLL(str(so))


def test_stages_give_the_doubles_of_the_whole(m):
    rng = np.random.default_rng(11)
    x = np.concatenate([-np.exp(rng.uniform(np.log(1e-300), np.log(1200), 200000)), rng.uniform(-40, 0, 100000),
                        [0.0, -0.0, -np.inf, -745.2, -1100.0, -1e5, -1e300, -5e-324, -np.log(2) / 64, -708.5]])
    outs = []
    for f in (m.whole, m.stages):
        y, z, w = np.zeros_like(x), np.zeros_like(x), np.zeros_like(x)
        f(len(x), x.ctypes.data_as(dp), y.ctypes.data_as(dp), z.ctypes.data_as(dp), w.ctypes.data_as(dp))
        outs.append((y, z, w))
    for a, b in zip(*outs):
        assert a.tobytes() == b.tobytes()
