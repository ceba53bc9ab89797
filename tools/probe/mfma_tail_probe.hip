// Development aid (round 7): is a chain of v_mfma_f32_4x4x1_16B_f32 over k the SAME BITS as v_mfma_f32_16x16x4_f32 over the same k in
// the same order, from the same starting accumulator?  (The gate of the 25th cell's tile of the 3x3 layers, ccsp_net.hip: tail_tile_4x4.)
// Both forms are compared bit for bit with a plain fmaf chain on the host and with each other, K = 64 and K = 80, in the order the
// network's layers use: k-block kb, MFMA step j, k-slot q -> k = 16 kb + 4 q + j (the 16x16x4 instruction adds its four k-slots in
// ascending q; the ascending-k order is compared too, for the record).  Inputs: fp32 of mixed magnitude, denormals, values whose
// products are denormal, signed zeros.  Also: the issue rate of ONE dependent chain of 4x4x1 instructions (the tail job is one).
//   hipcc --offload-arch=gfx950 -O2 -o mfma_tail_probe tools/probe/mfma_tail_probe.hip && ./mfma_tail_probe
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int ROWS = 8, COLS = 32;

// one wave per trial: A[trial][8][K], W[trial][K][32] -> out16 / out4 [trial][8][32]
template <int K>
__global__ __launch_bounds__(64) void chains(const float *__restrict__ A, const float *__restrict__ W, float *out16, float *out4, unsigned long long *cyc) {
    const int lane = threadIdx.x, t = blockIdx.x;
    const float *a = A + (size_t)t * ROWS * K, *w = W + (size_t)t * K * COLS;
    {   // the layers' form: weights first, activations second (transposed tile): lane (l15, q) ends up with row l15, columns 16 nt + 4 q + reg
        const int l15 = lane & 15, q = lane >> 4;
        for (int nt = 0; nt < 2; nt++) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            for (int kb = 0; kb < K / 16; kb++)
                for (int j = 0; j < 4; j++) {
                    const int k = 16 * kb + 4 * q + j;
                    const float av = l15 < ROWS ? a[l15 * K + k] : 0.0f, bv = w[k * COLS + 16 * nt + l15];
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(bv, av, acc, 0, 0, 0);
                }
            if (l15 < ROWS)
                for (int r = 0; r < 4; r++) out16[((size_t)t * ROWS + l15) * COLS + 16 * nt + 4 * q + r] = acc[r];
        }
    }
    {   // sixteen 4 x 4 blocks = 2 row groups x 8 column groups: lane supplies row 4 ((lane >> 2) & 1) + (lane & 3) and column
        // 4 (lane >> 3) + (lane & 3); reg r of the result is row 4 ((lane >> 2) & 1) + r of the lane's column
        const int row = 4 * ((lane >> 2) & 1) + (lane & 3), col = 4 * (lane >> 3) + (lane & 3);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int kb = 0; kb < K / 16; kb++)
            for (int j = 0; j < 4; j++)
                for (int q = 0; q < 4; q++) {
                    const int k = 16 * kb + 4 * q + j;
                    acc = __builtin_amdgcn_mfma_f32_4x4x1f32(a[row * K + k], w[k * COLS + col], acc, 0, 0, 0);
                }
        for (int r = 0; r < 4; r++) out4[((size_t)t * ROWS + 4 * ((lane >> 2) & 1) + r) * COLS + col] = acc[r];
    }
    if (t == 0 && K == 64) {    // one dependent chain of 256 instructions from registers
        f32x4 c = {0.f, 0.f, 0.f, 0.f};
        const float x = a[lane], y = w[lane];
        const unsigned long long t0 = __builtin_amdgcn_s_memtime();
#pragma unroll 16
        for (int i = 0; i < 256; i++) c = __builtin_amdgcn_mfma_f32_4x4x1f32(x, y, c, 0, 0, 0);
        const unsigned long long t1 = __builtin_amdgcn_s_memtime();
        if (c[0] + c[1] + c[2] + c[3] == 12345.678f) out4[0] = 0.f;     // (keeps the chain)
        if (lane == 0) cyc[0] = t1 - t0;
    }
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 16); }
static float from_bits(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }
static uint32_t bits_of(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }
static float draw(bool small) {              // small: nothing but zeros, denormals and values whose products are denormal -- so are the sums
    const uint32_t kind = rnd() % (small ? 3 : 16), sign = (rnd() & 1u) << 31, man = rnd() & 0x7FFFFFu;
    if (kind == 0) return from_bits(sign);                                      // +0 / -0
    if (kind == 1) return from_bits(sign | man);                                // a denormal
    if (kind == 2) return from_bits(sign | ((127u - 55u - rnd() % 20u) << 23) | man);   // 2^-75 .. 2^-55: products are denormal or vanish
    if (kind < 8) return from_bits(sign | ((127u - 20u + rnd() % 41u) << 23) | man);    // 2^-20 .. 2^20
    return from_bits(sign | ((127u - 3u + rnd() % 6u) << 23) | man);                    // the size of activations and weights
}

template <int K>
static bool run(int trials) {
    std::vector<float> A((size_t)trials * ROWS * K), W((size_t)trials * K * COLS);
    for (size_t i = 0; i < A.size(); i++) A[i] = draw((i / (ROWS * K)) % 4 == 3);        // every fourth trial: small values only
    for (size_t i = 0; i < W.size(); i++) W[i] = draw((i / (K * COLS)) % 4 == 3);
    float *dA, *dW, *d16, *d4; unsigned long long *dc;
    const size_t no = (size_t)trials * ROWS * COLS;
    hipMalloc(&dA, A.size() * 4); hipMalloc(&dW, W.size() * 4); hipMalloc(&d16, no * 4); hipMalloc(&d4, no * 4); hipMalloc(&dc, 8);
    hipMemcpy(dA, A.data(), A.size() * 4, hipMemcpyHostToDevice); hipMemcpy(dW, W.data(), W.size() * 4, hipMemcpyHostToDevice);
    hipMemset(d16, 0xFF, no * 4); hipMemset(d4, 0xFF, no * 4); hipMemset(dc, 0, 8);
    hipLaunchKernelGGL((chains<K>), dim3(trials), dim3(64), 0, 0, dA, dW, d16, d4, dc);
    if (hipDeviceSynchronize() != hipSuccess) { printf("K = %d: the kernel failed\n", K); return false; }
    std::vector<float> o16(no), o4(no);
    unsigned long long cyc = 0;
    hipMemcpy(o16.data(), d16, no * 4, hipMemcpyDeviceToHost); hipMemcpy(o4.data(), d4, no * 4, hipMemcpyDeviceToHost); hipMemcpy(&cyc, dc, 8, hipMemcpyDeviceToHost);
    size_t d_16_host = 0, d_4_host = 0, d_4_16 = 0, d_16_asc = 0, denorm_out = 0, zero_out = 0;
    for (int t = 0; t < trials; t++)
        for (int r = 0; r < ROWS; r++)
            for (int c = 0; c < COLS; c++) {
                const float *a = &A[((size_t)t * ROWS + r) * K], *w = &W[(size_t)t * K * COLS + c];
                float ref = 0.0f, asc = 0.0f;
                for (int kb = 0; kb < K / 16; kb++)
                    for (int j = 0; j < 4; j++)
                        for (int q = 0; q < 4; q++) { const int k = 16 * kb + 4 * q + j; ref = __builtin_fmaf(a[k], w[(size_t)k * COLS], ref); }
                for (int k = 0; k < K; k++) asc = __builtin_fmaf(a[k], w[(size_t)k * COLS], asc);
                const size_t i = ((size_t)t * ROWS + r) * COLS + c;
                const uint32_t b16 = bits_of(o16[i]), b4 = bits_of(o4[i]), bh = bits_of(ref);
                d_16_host += b16 != bh; d_4_host += b4 != bh; d_4_16 += b4 != b16; d_16_asc += b16 != bits_of(asc);
                denorm_out += (bh & 0x7F800000u) == 0 && (bh & 0x7FFFFFu) != 0; zero_out += (bh & 0x7FFFFFFFu) == 0;
            }
    printf("K = %d, %d trials x 8 rows x 32 columns = %zu outputs (%zu of the host's are denormal, %zu zero)\n", K, trials, no, denorm_out, zero_out);
    printf("  16x16x4 chain  != host fmaf chain (order kb, j, q): %zu\n", d_16_host);
    printf("  4x4x1 chain    != host fmaf chain (order kb, j, q): %zu\n", d_4_host);
    printf("  4x4x1 chain    != 16x16x4 chain                   : %zu   <- the gate\n", d_4_16);
    printf("  (16x16x4 chain != host fmaf chain in ascending k  : %zu -- the order matters, as expected)\n", d_16_asc);
    if (K == 64) printf("  one dependent chain of 256 v_mfma_f32_4x4x1: %llu ticks of s_memtime = %.1f each (8 when nothing depends)\n", cyc, cyc / 256.0);
    hipFree(dA); hipFree(dW); hipFree(d16); hipFree(d4); hipFree(dc);
    return d_4_16 == 0;
}

int main() {
    const bool ok64 = run<64>(512), ok80 = run<80>(512);
    printf("gate: %s\n", ok64 && ok80 ? "PASS -- the two instructions form the same bits" : "FAIL -- the bits differ");
    return ok64 && ok80 ? 0 : 1;
}
