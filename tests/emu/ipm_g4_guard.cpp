// Host-side probe of the register-resident interior-point kernel's launch guard (alqp_ipm_g4_launch.hpp):
// the admissibility predicate alone, compiled without HIP and called through ctypes (tests/test_ipm_g4_guard.py).
// TEST INFRASTRUCTURE: the product path never loads this.
#include "alqp_ipm_g4_launch.hpp"

extern "C" int g4_resident_addressable(int T, int nx, int nu, int real_bytes, long sC_t, long sF_t, long sf_t) {
    return alqp_ipm_g4::resident_addressable(T, nx, nu, real_bytes, sC_t, sF_t, sf_t) ? 1 : 0;
}
