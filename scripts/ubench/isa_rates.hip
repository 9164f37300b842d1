// Issue-rate microbenchmark for the integer VALU instructions the field
// kernels lean on (gfx950).  8 independent dependency chains per lane, inline
// asm so the exact instruction is issued.  Prints ns per wave-instruction per
// SIMD (lower is better) and the implied cycles at the measured clock.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdint.h>

#define ITERS 4096

#define CHAIN8(ASM)                                                                 \
    asm volatile(ASM : "+v"(a0) : "v"(k)); asm volatile(ASM : "+v"(a1) : "v"(k));  \
    asm volatile(ASM : "+v"(a2) : "v"(k)); asm volatile(ASM : "+v"(a3) : "v"(k));  \
    asm volatile(ASM : "+v"(a4) : "v"(k)); asm volatile(ASM : "+v"(a5) : "v"(k));  \
    asm volatile(ASM : "+v"(a6) : "v"(k)); asm volatile(ASM : "+v"(a7) : "v"(k));

// The FD step's operand shape: vdst = v_bits * s_const + v_bits, the vector
// operands small-integer bit patterns (f32 subnormals), the constant a normal
// float in an SGPR, every result an integer in [0, 2^24].  The eight
// destinations are independent (at 8 waves per SIMD the issue rate does not
// depend on the chains); rows 32..34 are the integer forms in the same shape.
#define IND8V(ASM, c, K, t)                                                                             \
    asm volatile(ASM : "=v"(a0) : "v"(c), "s"(K), "v"(t)); asm volatile(ASM : "=v"(a1) : "v"(c), "s"(K), "v"(t));  \
    asm volatile(ASM : "=v"(a2) : "v"(c), "s"(K), "v"(t)); asm volatile(ASM : "=v"(a3) : "v"(c), "s"(K), "v"(t));  \
    asm volatile(ASM : "=v"(a4) : "v"(c), "s"(K), "v"(t)); asm volatile(ASM : "=v"(a5) : "v"(c), "s"(K), "v"(t));  \
    asm volatile(ASM : "=v"(a6) : "v"(c), "s"(K), "v"(t)); asm volatile(ASM : "=v"(a7) : "v"(c), "s"(K), "v"(t));  \
    asm volatile("" ::"v"(a0), "v"(a1), "v"(a2), "v"(a3), "v"(a4), "v"(a5), "v"(a6), "v"(a7));  /* eight live registers */
#define IND8(ASM, K) IND8V(ASM, c, K, t)

// The eight registers as accumulators: vdst is also the addend.
#define ACC8(ASM, C, K)                                                                          \
    asm volatile(ASM : "+v"(a0) : "v"(C), K); asm volatile(ASM : "+v"(a1) : "v"(C), K);          \
    asm volatile(ASM : "+v"(a2) : "v"(C), K); asm volatile(ASM : "+v"(a3) : "v"(C), K);          \
    asm volatile(ASM : "+v"(a4) : "v"(C), K); asm volatile(ASM : "+v"(a5) : "v"(C), K);          \
    asm volatile(ASM : "+v"(a6) : "v"(C), K); asm volatile(ASM : "+v"(a7) : "v"(C), K);

template <int OP>
__global__ void kern(uint32_t *out, uint32_t seed) {
    uint32_t k = seed + threadIdx.x;
    uint32_t a0 = k, a1 = k + 1, a2 = k + 2, a3 = k + 3, a4 = k + 4, a5 = k + 5, a6 = k + 6, a7 = k + 7;
    for (int i = 0; i < ITERS; i++) {
        if constexpr (OP == 0) { CHAIN8("v_add_u32 %0, %0, %1") }
        if constexpr (OP == 1) { CHAIN8("v_sub_u32 %0, %0, %1") }
        if constexpr (OP == 2) { CHAIN8("v_or_b32 %0, %0, %1") }
        if constexpr (OP == 3) { CHAIN8("v_and_b32 %0, %0, %1") }
        if constexpr (OP == 4) { CHAIN8("v_xor_b32 %0, %0, %1") }
        if constexpr (OP == 5) { CHAIN8("v_lshrrev_b32 %0, %1, %0") }
        if constexpr (OP == 6) { CHAIN8("v_lshlrev_b32 %0, %1, %0") }
        if constexpr (OP == 7) { CHAIN8("v_add3_u32 %0, %0, %1, %0") }
        if constexpr (OP == 8) { CHAIN8("v_or3_b32 %0, %0, %1, %0") }
        if constexpr (OP == 9) { CHAIN8("v_mul_u32_u24 %0, %0, %1") }
        if constexpr (OP == 10) { CHAIN8("v_mad_u32_u24 %0, %0, %1, %0") }
        if constexpr (OP == 11) { CHAIN8("v_mad_i32_i24 %0, %0, %1, %0") }
        if constexpr (OP == 12) { CHAIN8("v_mul_hi_u32 %0, %0, %1") }
        if constexpr (OP == 13) { CHAIN8("v_mul_lo_u32 %0, %0, %1") }
        if constexpr (OP == 14) { CHAIN8("v_bcnt_u32_b32 %0, %0, %1") }
        if constexpr (OP == 15) { CHAIN8("v_bfe_u32 %0, %0, %1, 5") }
        if constexpr (OP == 16) { CHAIN8("v_lshl_add_u32 %0, %0, 3, %1") }
        if constexpr (OP == 17) { CHAIN8("v_min_u32 %0, %0, %1") }
        if constexpr (OP == 18) { CHAIN8("v_pk_add_u16 %0, %0, %1") }
        if constexpr (OP == 19) { CHAIN8("v_pk_mad_u16 %0, %0, %1, %0") }
        if constexpr (OP == 20) { CHAIN8("v_pk_lshrrev_b16 %0, %1, %0") }
        if constexpr (OP == 21) { CHAIN8("v_add_f32 %0, %0, %1") }
        if constexpr (OP == 22) { CHAIN8("v_fma_f32 %0, %0, %1, %0") }
        if constexpr (OP == 23) { CHAIN8("v_pk_add_u16 %0, %0, %1") }
        if constexpr (OP == 24) { CHAIN8("v_add_u32 %0, %0, %1") }
        if constexpr (OP == 25) { CHAIN8("v_mov_b32 %0, %1") }
        if constexpr (OP == 26) { CHAIN8("v_add_u32_e64 %0, %0, %1") }
        if constexpr (OP >= 27) {
            const uint32_t c = (k & 3) + 1, t = 5 * 12800 + (k & 63);  // carry 1..4, limb sum
            if constexpr (OP == 27) { IND8("v_fma_f32 %0, %1, %2, %3", 3.0f) }
            if constexpr (OP == 28) { IND8("v_fma_f32 %0, %1, %2, %3", 8.0f) }
            if constexpr (OP == 29) { IND8("v_fma_f32 %0, %1, %2, %3", -12800.0f) }
            if constexpr (OP == 30) { IND8("v_mul_f32 %0, %2, %1 ; %3", 8.0f) }
            if constexpr (OP == 31) {  // accumulates 3 c per iteration: < 2^24 after ITERS
                asm volatile("v_fmac_f32 %0, %2, %1" : "+v"(a0) : "v"(c), "s"(3.0f)); asm volatile("v_fmac_f32 %0, %2, %1" : "+v"(a1) : "v"(c), "s"(3.0f));
                asm volatile("v_fmac_f32 %0, %2, %1" : "+v"(a2) : "v"(c), "s"(3.0f)); asm volatile("v_fmac_f32 %0, %2, %1" : "+v"(a3) : "v"(c), "s"(3.0f));
                asm volatile("v_fmac_f32 %0, %2, %1" : "+v"(a4) : "v"(c), "s"(3.0f)); asm volatile("v_fmac_f32 %0, %2, %1" : "+v"(a5) : "v"(c), "s"(3.0f));
                asm volatile("v_fmac_f32 %0, %2, %1" : "+v"(a6) : "v"(c), "s"(3.0f)); asm volatile("v_fmac_f32 %0, %2, %1" : "+v"(a7) : "v"(c), "s"(3.0f));
            }
            if constexpr (OP == 32) { IND8("v_mad_u32_u24 %0, %1, %2, %3", 3) }
            if constexpr (OP == 33) { IND8("v_mad_i32_i24 %0, %1, %2, %3", -12800) }
            if constexpr (OP == 34) { IND8("v_lshl_add_u32 %0, %1, 3, %3 ; %2", 8) }
            // What sets the f32 rows above apart from row 22: the constant's
            // place (35 VGPR, 36 inline), subnormal against normal operands
            // (37, 40), the destination being a source (38..40), or three
            // distinct registers at all (41..43: the 2.5-cycle adds reshaped).
            const uint32_t kv = __float_as_uint(3.0f) + (k >> 30);  // 3.0f in a VGPR
            const uint32_t cn = __float_as_uint((float)c), tn = __float_as_uint((float)t);
            if constexpr (OP == 35) { IND8("v_fma_f32 %0, %1, %2, %3", kv) }
            if constexpr (OP == 36) { IND8("v_fma_f32 %0, %1, 4.0, %3 ; %2", 0) }
            if constexpr (OP == 37) { IND8V("v_fma_f32 %0, %1, %2, %3", cn, -12800.0f, tn) }
            if constexpr (OP == 38) { ACC8("v_fma_f32 %0, %1, %2, %0", c, "s"(3.0f)) }
            if constexpr (OP == 39) { ACC8("v_fma_f32 %0, %1, %2, %0", c, "v"(kv)) }
            if constexpr (OP == 40) {
                if (i == 0) { a0 = a1 = a2 = a3 = a4 = a5 = a6 = a7 = tn; }
                ACC8("v_fma_f32 %0, %1, %2, %0", cn, "v"(kv))
            }
            if constexpr (OP == 41) { IND8("v_add_f32 %0, %1, %3 ; %2", 0) }
            if constexpr (OP == 42) { IND8("v_add_u32 %0, %1, %3 ; %2", 0) }
            if constexpr (OP == 43) { IND8("v_add_u32 %0, %2, %3 ; %1", seed) }
        }
    }
    out[blockIdx.x * blockDim.x + threadIdx.x] = a0 ^ a1 ^ a2 ^ a3 ^ a4 ^ a5 ^ a6 ^ a7;
}

// 64-bit shift: separate kernel (64-bit operands)
__global__ void kern_shl64(uint64_t *out, uint32_t seed) {
    uint32_t k = (seed + threadIdx.x) & 63;
    uint64_t a0 = k, a1 = k + 1, a2 = k + 2, a3 = k + 3, a4 = k + 4, a5 = k + 5, a6 = k + 6, a7 = k + 7;
    for (int i = 0; i < ITERS; i++) {
#define S64(a) asm volatile("v_lshlrev_b64 %0, %1, %0" : "+v"(a) : "v"(k));
        S64(a0) S64(a1) S64(a2) S64(a3) S64(a4) S64(a5) S64(a6) S64(a7)
    }
    out[blockIdx.x * blockDim.x + threadIdx.x] = a0 ^ a1 ^ a2 ^ a3 ^ a4 ^ a5 ^ a6 ^ a7;
}
// LDS random ds_read_b64 vs conflict-free, as issued by 16 waves/CU
__global__ void kern_lds(uint64_t *out, uint32_t seed, int random) {
    __shared__ uint64_t tab[1600];
    for (int i = threadIdx.x; i < 1600; i += blockDim.x) tab[i] = i * 0x9E3779B97F4A7C15ull;
    __syncthreads();
    uint32_t x = (seed + threadIdx.x * 2654435761u);
    uint64_t acc = 0;
    for (int i = 0; i < ITERS; i++) {
        uint32_t idx = random ? (x >> 16) % 1600 : (threadIdx.x + i) % 1600;
        x = x * 1664525u + 1013904223u;
        acc ^= tab[idx];
    }
    out[blockIdx.x * blockDim.x + threadIdx.x] = acc;
}

int main() {
    uint64_t *buf;
    hipMalloc(&buf, 256 * 1024 * 1024);
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    const int grid = 256 * 8, block = 256;  // 8 WGs/CU -> 8 waves/SIMD
    const char *names[] = {"v_add_u32","v_sub_u32","v_or_b32","v_and_b32","v_xor_b32","v_lshrrev_b32","v_lshlrev_b32","v_add3_u32","v_or3_b32","v_mul_u32_u24","v_mad_u32_u24","v_mad_i32_i24","v_mul_hi_u32","v_mul_lo_u32","v_bcnt_u32_b32","v_bfe_u32","v_lshl_add_u32","v_min_u32","v_pk_add_u16","v_pk_mad_u16","v_pk_lshrrev_b16","v_add_f32","v_fma_f32","v_pk_add_u16_b","v_add_u32_b","v_mov_b32","v_add_u32_e64",
        "v_fma_f32 v,s3.0,v","v_fma_f32 v,s8.0,v","v_fma_f32 v,s-12800,v","v_mul_f32 s8.0,v","v_fmac_f32 s3.0,v",
        "v_mad_u32_u24 v,s,v","v_mad_i32_i24 v,s,v","v_lshl_add_u32 v,3,v",
        "v_fma_f32 v,vK,v","v_fma_f32 v,4.0,v","v_fma_f32 v,s,v normal","v_fma_f32 acc v,s","v_fma_f32 acc v,vK","v_fma_f32 acc normal",
        "v_add_f32 d,v,v","v_add_u32 d,v,v","v_add_u32 d,s,v"};
    auto run = [&](auto launch, const char *name) {
        launch();
        hipDeviceSynchronize();
        hipEventRecord(e0);
        launch();
        hipEventRecord(e1);
        hipEventSynchronize(e1);
        float ms;
        hipEventElapsedTime(&ms, e0, e1);
        double winstr = (double)grid * block / 64 * ITERS * 8;  // wave-instructions
        double per_simd = winstr / 1024;
        printf("%-22s %8.3f ms  %.3f ns per wave-instr per SIMD (%.2f cyc @2.4GHz)\n", name, ms,
               ms * 1e6 / per_simd, ms * 1e6 / per_simd * 2.4);
    };
#define RUN(OP) run([&] { hipLaunchKernelGGL(kern<OP>, dim3(grid), dim3(block), 0, 0, (uint32_t *)buf, 7u); }, names[OP]);
    RUN(0) RUN(1) RUN(2) RUN(3) RUN(4) RUN(5) RUN(6) RUN(7) RUN(8) RUN(9) RUN(10) RUN(11) RUN(12) RUN(13) RUN(14) RUN(15) RUN(16) RUN(17) RUN(18) RUN(19) RUN(20) RUN(21) RUN(22) RUN(23) RUN(24) RUN(25) RUN(26)
    RUN(27) RUN(28) RUN(29) RUN(30) RUN(31) RUN(32) RUN(33) RUN(34)
    RUN(35) RUN(36) RUN(37) RUN(38) RUN(39) RUN(40) RUN(41) RUN(42) RUN(43)
    run([&] { hipLaunchKernelGGL(kern_shl64, dim3(grid), dim3(block), 0, 0, buf, 7u); }, "v_lshlrev_b64");
    for (int r = 0; r < 2; r++) {
        hipLaunchKernelGGL(kern_lds, dim3(grid), dim3(block), 0, 0, buf, 7u, r);
        hipDeviceSynchronize();
        hipEventRecord(e0);
        hipLaunchKernelGGL(kern_lds, dim3(grid), dim3(block), 0, 0, buf, 7u, r);
        hipEventRecord(e1);
        hipEventSynchronize(e1);
        float ms;
        hipEventElapsedTime(&ms, e0, e1);
        double lds_per_cu = (double)grid * block / 64 * ITERS / 256;
        printf("ds_read_b64 %s: %.3f ms, %.2f cyc per wave-read per CU @2.4GHz\n",
               r ? "random" : "linear", ms, ms * 1e6 * 2.4 / lds_per_cu);
    }
    return 0;
}
