// pbound_host.inc -- host side of Raghavan's bound of the statistical test (included by isocon_hip.hip): isocon_raghavan_bound.  No store, no
// handle: the two sums of every test go up as one image, the bounds' bits and the certificates come back through a slot of the process'
// scratch pool.  One launch (pbound.hpp).

extern "C" int isocon_raghavan_bound(const double *m_sum, const double *y_sum, uint64_t n, double *out_bound, uint8_t *out_certified, float *kernel_ms)
{
    if (kernel_ms) *kernel_ms = 0.f;
    if (!n) return ISOCON_OK;
    if (!m_sum || !y_sum || !out_bound || !out_certified) return ISOCON_E_ARG;
    if (n > ((uint64_t)1 << 32)) { g_last_error = "isocon_raghavan_bound: more than 2^32 tests in one call"; return ISOCON_E_ARG; }
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) { (void)hipGetLastError(); g_last_error = "isocon_raghavan_bound: no device"; return ISOCON_E_NODEVICE; }
    const size_t o_m = 0, o_y = (size_t)n * 8, a_bits = 0, a_cert = (size_t)n * 8;
    DevBuf d_in(&g_scratch, SLOT_PB_IN), d_out(&g_scratch, SLOT_PB_OUT);
    int rc;
    if ((rc = d_in.alloc((size_t)n * 16)) || (rc = d_out.alloc((size_t)n * 9))) return rc;
    uint8_t *in = d_in.as<uint8_t>(), *out = d_out.as<uint8_t>();
    ISO_HIP_CHECK(copy_h2d(in + o_m, m_sum, (size_t)n * 8));
    ISO_HIP_CHECK(copy_h2d(in + o_y, y_sum, (size_t)n * 8));
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((n + 255) / 256, 1u << 16);
    EventTimer tm;
    tm.start();
    hipLaunchKernelGGL(k_pvalue_bound, dim3(blocks), dim3(256), 0, 0, (const uint64_t *)(in + o_m), (const uint64_t *)(in + o_y), n, (uint64_t *)(out + a_bits), out + a_cert);
    ISO_HIP_CHECK(hipGetLastError());
    tm.stop();
    if (kernel_ms) *kernel_ms = tm.total;
    ISO_HIP_CHECK(copy_d2h(out_bound, out + a_bits, (size_t)n * 8));
    ISO_HIP_CHECK(copy_d2h(out_certified, out + a_cert, (size_t)n));
    return ISOCON_OK;
}
