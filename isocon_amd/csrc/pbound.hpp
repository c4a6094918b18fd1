// pbound.hpp -- kernel of Raghavan's bound of the statistical test (isocon_raghavan_bound: pbound_host.inc; lane math in pbound_core.hpp).
// Reference call site: modules/hypothesis_test_module.py:253-329.
//
//   k_pvalue_bound   one lane per test, 256 threads per workgroup, a grid-stride loop: two 8-byte loads (the bits of m_sum and y_sum), the
//                    320-bit fixed-point evaluation of pb_eval, one 8-byte store (the bound's bits) and one byte store (certified).
// No LDS, no scratch, no cross-lane traffic, no floating-point instruction, no inline assembly.
#pragma once
#include "common.hpp"
#include "pbound_core.hpp"

namespace isocon {

__global__ __launch_bounds__(256) void k_pvalue_bound(const uint64_t *__restrict__ m_bits, const uint64_t *__restrict__ y_bits, uint64_t n,
                                                      uint64_t *__restrict__ out_bits, uint8_t *__restrict__ out_certified)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        uint8_t certified;
        out_bits[i] = pb_eval(m_bits[i], y_bits[i], &certified);
        out_certified[i] = certified;
    }
}

}  // namespace isocon
