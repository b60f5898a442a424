// How good is v_rcp_f64 as the seed of the SHARED reciprocal of k_jump_bin's paired step (hulk_spectrum.hip)?
// The loop feeds it P = RN(x_a * x_b), x = r * 2^-31, r = (key >> 33) + 1 of two consecutive LCG keys.  Measured here, as the
// largest |1 - P * rho| (one fma: the residual is exact up to its own rounding) over
//   * 2^30 pairs (r_a, r_b) from the loop's own LCG, 1024 consecutive pairs per thread from a hashed start key,
//   * every single r in [1, 2^31] (x_b = 1),
// for the bare seed and after one and two Newton steps; and end to end, the largest |1 - x_a * q_a| and |1 - x_b * q_b| of
// q_a = RN(rho * x_b), q_b = RN(rho * x_a), which is the relative error the step's product inherits.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
struct Worst { unsigned long long seed, rho[2], q[2]; };     // bits of non-negative doubles: they order like the doubles
__device__ __forceinline__ void upd(unsigned long long &w, double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(fabs(v));
    if (b > w) w = b;
}
__device__ __forceinline__ void one(Worst &w, uint32_t ra_m1, uint32_t rb_m1) {
    const double xa = ((double)ra_m1 + 1.0) * 0x1p-31, xb = ((double)rb_m1 + 1.0) * 0x1p-31;
    const double P = xa * xb;
    double rho = __builtin_amdgcn_rcp(P);
    upd(w.seed, __builtin_fma(-P, rho, 1.0));
    for (int s = 0; s < 2; s++) {
        const double e = __builtin_fma(-P, rho, 1.0);
        rho = __builtin_fma(rho, e, rho);
        upd(w.rho[s], __builtin_fma(-P, rho, 1.0));
        const double qa = rho * xb, qb = rho * xa;
        upd(w.q[s], __builtin_fma(-xa, qa, 1.0));
        upd(w.q[s], __builtin_fma(-xb, qb, 1.0));
    }
}
__device__ void flush(Worst *out, const Worst &w) {
    atomicMax(&out->seed, w.seed);
    for (int s = 0; s < 2; s++) { atomicMax(&out->rho[s], w.rho[s]); atomicMax(&out->q[s], w.q[s]); }
}
__global__ void k_pairs(Worst *out, int per_thread) {
    Worst w{};
    uint64_t key = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x + 1) * 0x9E3779B97F4A7C15ull;
    key ^= key >> 29; key *= 0xBF58476D1CE4E5B9ull; key ^= key >> 32;
    for (int i = 0; i < per_thread; i++) {
        key = key * 2862933555777941757ull + 1;
        const uint32_t a = (uint32_t)(key >> 33);
        key = key * 2862933555777941757ull + 1;
        one(w, a, (uint32_t)(key >> 33));
    }
    flush(out, w);
}
__global__ void k_singles(Worst *out) {
    Worst w{};
    for (uint64_t m = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; m < 0x80000000ull; m += (uint64_t)gridDim.x * blockDim.x)
        one(w, (uint32_t)m, 0x7FFFFFFFu);
    flush(out, w);
}
static void report(const char *what, Worst *d) {
    Worst h;
    hipMemcpy(&h, d, sizeof h, hipMemcpyDeviceToHost);
    auto lg = [](unsigned long long b) { double v; memcpy(&v, &b, 8); return v > 0 ? log2(v) : -INFINITY; };
    printf("%s: seed 2^%.2f | 1 Newton step: rho 2^%.2f, q 2^%.2f | 2 steps: rho 2^%.2f, q 2^%.2f\n", what, lg(h.seed),
           lg(h.rho[0]), lg(h.q[0]), lg(h.rho[1]), lg(h.q[1]));
    hipMemset(d, 0, sizeof h);
}
int main() {
    Worst *d;
    if (hipMalloc(&d, sizeof(Worst)) != hipSuccess) return 1;
    hipMemset(d, 0, sizeof(Worst));
    k_pairs<<<4096, 256>>>(d, 1024);
    if (hipDeviceSynchronize() != hipSuccess) return 1;
    report("2^30 LCG pairs      ", d);
    k_singles<<<4096, 256>>>(d);
    if (hipDeviceSynchronize() != hipSuccess) return 1;
    report("every r in [1, 2^31]", d);
    hipFree(d);
    return 0;
}
