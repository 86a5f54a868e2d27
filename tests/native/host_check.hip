// host_check.hip -- a stand-alone check of the host-only helpers of csrc/svdq_small_view.h and csrc/svdq_store_pass.h
// (tests/test_host_helpers_cpu.py builds it with the address and undefined-behaviour sanitizers on the host side and runs
// it; no GPU, no HIP call).  Views over layouts made by svdq_small_layout_of are compared, array by array, with the casts
// the launchers used to write by hand; the slot class and the block geometry with the expressions the launchers and
// kernels carried; the refusal helpers with the texts the entry points set.
#include "svdq_small_view.h"
#include "svdq_store_pass.h"

#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <vector>

static char g_err[512];
void svdq_set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

static int failures = 0;
static void fail(int line, const char *what) {
    printf("host_check.hip:%d: %s\n", line, what);
    ++failures;
}
#define CHECK(c) ((c) ? (void)0 : fail(__LINE__, #c))

static int64_t up64(int64_t x) { return (x + 63) / 64 * 64; }

int main() {
    for (int64_t P : {1, 3, 296})
        for (int64_t N : {1, 8, 17, 32})
            for (int64_t S : {1, 2, 4}) {
                const svdq_small_layout L = svdq_small_layout_of(P, N, S);
                // the layout svdq_plan_create wrote out line by line
                int64_t off = 0;
                CHECK(L.sigma_off == off), off += up64(P * N * 4);
                CHECK(L.k_off == off), off += up64(P * 4);
                CHECK(L.r_off == off), off += up64(P * 4);
                CHECK(L.energy_off == off), off += up64(P * 4);
                CHECK(L.rows_off == off), off += up64(P * 8);
                CHECK(L.chigh_off == off), off += up64(P * N * N * 2);
                CHECK(L.codes_off == off), off += up64(P * N * S * N);
                CHECK(L.scale_off == off), off += up64(P * N * S * 4);
                CHECK(L.zp_off == off), off += up64(P * N * S * 4);
                CHECK(L.rnorm_off == off), off += up64(P * N * S * 4);
                CHECK(L.coef_off == off), off += up64(P * N * N * 4);
                CHECK(L.status_off == off), off += 64;
                CHECK(L.total_bytes == off);

                std::vector<uint8_t> buf((size_t)L.total_bytes, 0);
                uint8_t *sm = buf.data();
                const SmallViewMut w = small_view_mut(L, sm);
                const SmallView c = small_view(L, sm);
                CHECK(w.sigma == reinterpret_cast<float *>(sm + L.sigma_off) && c.sigma == w.sigma);
                CHECK(w.k == reinterpret_cast<int32_t *>(sm + L.k_off) && c.k == w.k);
                CHECK(w.r == reinterpret_cast<int32_t *>(sm + L.r_off) && c.r == w.r);
                CHECK(w.energy == reinterpret_cast<float *>(sm + L.energy_off) && c.energy == w.energy);
                CHECK(w.rows == reinterpret_cast<int64_t *>(sm + L.rows_off) && c.rows == w.rows);
                CHECK(w.chigh == reinterpret_cast<uint16_t *>(sm + L.chigh_off) && c.chigh == w.chigh);
                CHECK(w.codes == sm + L.codes_off && c.codes == w.codes);
                CHECK(w.scale == reinterpret_cast<float *>(sm + L.scale_off) && c.scale == w.scale);
                CHECK(w.zp == reinterpret_cast<float *>(sm + L.zp_off) && c.zp == w.zp);
                CHECK(w.rnorm == reinterpret_cast<float *>(sm + L.rnorm_off) && c.rnorm == w.rnorm);
                CHECK(w.coef == reinterpret_cast<float *>(sm + L.coef_off) && c.coef == w.coef);
                CHECK(w.status == reinterpret_cast<int32_t *>(sm + L.status_off) && c.status == w.status);
                // every array's last element lies inside the buffer (the sanitizer watches the writes)
                w.sigma[P * N - 1] = 1.f, w.k[P - 1] = 1, w.r[P - 1] = 1, w.energy[P - 1] = 1.f, w.rows[P - 1] = 1;
                w.chigh[P * N * N - 1] = 1, w.codes[P * N * S * N - 1] = 1, w.scale[P * N * S - 1] = 1.f;
                w.zp[P * N * S - 1] = 1.f, w.rnorm[P * N * S - 1] = 1.f, w.coef[P * N * N - 1] = 1.f, w.status[0] = 1;
            }

    // slot class and block geometry against what the launchers and the kernels each wrote
    for (int n = 1; n <= 32; ++n) {
        const int cls = svdq_slot_class(n);
        CHECK(cls == (n <= 8 ? 8 : (n <= 16 ? 16 : 32)));
        CHECK(store_rb(cls) == (cls <= 16 ? 256 : 128) && store_rpl(cls) == (cls > 16 ? 2 : 4));
        for (int es : {2, 4}) CHECK(store_sv(cls, es) == (store_rb(cls) * cls * es / 16 + 2 + 63) / 64);
    }

    // the refusals: what passes, what is refused, and the texts byte for byte
    svdq_plan pl;
    memset(&pl, 0, sizeof pl);
    float mean[4];
    CHECK(!svdq_refuse_no_mean("f", &pl, nullptr));
    pl.cfg.center = 1;
    CHECK(!svdq_refuse_no_mean("f", &pl, mean));
    CHECK(svdq_refuse_no_mean("svdq_plan_project", &pl, nullptr));
    CHECK(!strcmp(g_err, "svdq_plan_project: mean is required on a centred plan"));
    alignas(16) uint8_t a[32];
    CHECK(svdq_addr_bits(a, nullptr, a + 16) == ((uintptr_t)a | (uintptr_t)(a + 16)));
    CHECK(!svdq_refuse_unaligned("f", svdq_addr_bits(a, nullptr, a + 8), 8, "x"));
    CHECK(!svdq_refuse_unaligned("f", svdq_addr_bits(a, a + 16), 16, "x"));
    CHECK(svdq_refuse_unaligned("svdq_plan_project", svdq_addr_bits(a, a + 4), 8, "pointer tables, rows and work"));
    CHECK(!strcmp(g_err, "svdq_plan_project: pointer tables, rows and work must be 8-byte aligned"));
    CHECK(svdq_refuse_unaligned("svdq_plan_extend_basis", svdq_addr_bits(a + 4), 8, "pointer tables, rows and ", "out_ptrs"));
    CHECK(!strcmp(g_err, "svdq_plan_extend_basis: pointer tables, rows and out_ptrs must be 8-byte aligned"));
    CHECK(svdq_refuse_unaligned("svdq_plan_store_gram", svdq_addr_bits(a, a + 8), 16, "small, basis and mean"));
    CHECK(!strcmp(g_err, "svdq_plan_store_gram: small, basis and mean must be 16-byte aligned"));

    printf(failures ? "host_check: %d FAILED\n" : "host_check: ok\n", failures);
    return failures ? 1 : 0;
}
