// issue_rates.hip — diagnostic microbenchmark (not part of the product): wave-instruction issue rates on gfx950 as a function
// of waves per SIMD, for the instruction classes the QRMSA kernel is made of.  Build: hipcc --offload-arch=gfx950 -O3 -o issue_rates issue_rates.hip
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <algorithm>
#include <cstring>
#include <cstdint>

#define REP 64
#define ITERS 2000

// each kernel: ITERS iterations of REP instructions of one class; out keeps the compiler honest
#define KERNEL(name, decl, body)                                                           \
    __global__ __launch_bounds__(64) void name(unsigned long long *out, int iters) {                            \
        decl;                                                                               \
        for (int it = 0; it < iters; ++it) {                                                \
            _Pragma("unroll") for (int r = 0; r < REP / 4; ++r) { body; }                   \
        }                                                                                   \
        FIN;                                                                                \
    }

// ---- VALU 32-bit add: 4 independent chains
#define FIN out[blockIdx.x * 64 + threadIdx.x] = (unsigned long long)(a0 + a1 + a2 + a3)
KERNEL(k_valu32, unsigned a0 = threadIdx.x; unsigned a1 = 1; unsigned a2 = 2; unsigned a3 = 3,
       asm volatile("v_add_u32 %0, %0, %0\n v_add_u32 %1, %1, %1\n v_add_u32 %2, %2, %2\n v_add_u32 %3, %3, %3"
                    : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3)))
// dependent chain (one register)
KERNEL(k_valu32_dep, unsigned a0 = threadIdx.x; unsigned a1 = 1; unsigned a2 = 2; unsigned a3 = 3,
       asm volatile("v_add_u32 %0, %0, %0\n v_add_u32 %0, %0, %0\n v_add_u32 %0, %0, %0\n v_add_u32 %0, %0, %0"
                    : "+v"(a0)))
#undef FIN
#define FIN out[blockIdx.x * 64 + threadIdx.x] = (unsigned long long)(a0 + a1 + a2 + a3)
KERNEL(k_shl64, unsigned long long a0 = threadIdx.x; unsigned long long a1 = 1; unsigned long long a2 = 2; unsigned long long a3 = 3,
       asm volatile("v_lshlrev_b64 %0, 1, %0\n v_lshlrev_b64 %1, 1, %1\n v_lshlrev_b64 %2, 1, %2\n v_lshlrev_b64 %3, 1, %3"
                    : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3)))
#undef FIN
#define FIN out[blockIdx.x * 64 + threadIdx.x] = (unsigned long long)(a0 + a1 + a2 + a3)
KERNEL(k_fma64, double a0 = threadIdx.x; double a1 = 1; double a2 = 2; double a3 = 3,
       asm volatile("v_fma_f64 %0, %0, %0, %0\n v_fma_f64 %1, %1, %1, %1\n v_fma_f64 %2, %2, %2, %2\n v_fma_f64 %3, %3, %3, %3"
                    : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3)))
KERNEL(k_add64f, double a0 = threadIdx.x; double a1 = 1; double a2 = 2; double a3 = 3,
       asm volatile("v_add_f64 %0, %0, %0\n v_add_f64 %1, %1, %1\n v_add_f64 %2, %2, %2\n v_add_f64 %3, %3, %3"
                    : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3)))
#undef FIN
#define FIN out[blockIdx.x * 64 + threadIdx.x] = (unsigned long long)(a0 + a1 + a2 + a3)
KERNEL(k_mullo, unsigned a0 = threadIdx.x; unsigned a1 = 1; unsigned a2 = 2; unsigned a3 = 3,
       asm volatile("v_mul_lo_u32 %0, %0, %0\n v_mul_lo_u32 %1, %1, %1\n v_mul_lo_u32 %2, %2, %2\n v_mul_lo_u32 %3, %3, %3"
                    : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3)))
KERNEL(k_dppmov, unsigned a0 = threadIdx.x; unsigned a1 = 1; unsigned a2 = 2; unsigned a3 = 3,
       asm volatile("v_mov_b32_dpp %0, %0 row_shl:1 row_mask:0xf bank_mask:0xf\n v_mov_b32_dpp %1, %1 row_shl:1 row_mask:0xf bank_mask:0xf\n"
                    "v_mov_b32_dpp %2, %2 row_shl:1 row_mask:0xf bank_mask:0xf\n v_mov_b32_dpp %3, %3 row_shl:1 row_mask:0xf bank_mask:0xf"
                    : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3)))
KERNEL(k_alignbit, unsigned a0 = threadIdx.x; unsigned a1 = 1; unsigned a2 = 2; unsigned a3 = 3,
       asm volatile("v_alignbit_b32 %0, %0, %1, 3\n v_alignbit_b32 %1, %1, %2, 3\n v_alignbit_b32 %2, %2, %3, 3\n v_alignbit_b32 %3, %3, %0, 3"
                    : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3)))
#undef FIN
// ---- SALU: 4 independent s_add
#define FIN out[blockIdx.x * 64 + threadIdx.x] = (unsigned long long)(s0 + s1 + s2 + s3)
KERNEL(k_salu, unsigned s0 = blockIdx.x; unsigned s1 = 1; unsigned s2 = 2; unsigned s3 = 3,
       asm volatile("s_add_u32 %0, %0, %0\n s_add_u32 %1, %1, %1\n s_add_u32 %2, %2, %2\n s_add_u32 %3, %3, %3"
                    : "+s"(s0), "+s"(s1), "+s"(s2), "+s"(s3) : : "scc"))
#undef FIN
// ---- mixed: 2 VALU + 2 SALU interleaved
#define FIN out[blockIdx.x * 64 + threadIdx.x] = (unsigned long long)(a0 + a1 + s0 + s1)
KERNEL(k_mixed, unsigned a0 = threadIdx.x; unsigned a1 = 1; unsigned s0 = blockIdx.x; unsigned s1 = 3,
       asm volatile("v_add_u32 %0, %0, %0\n s_add_u32 %2, %2, %2\n v_add_u32 %1, %1, %1\n s_add_u32 %3, %3, %3"
                    : "+v"(a0), "+v"(a1), "+s"(s0), "+s"(s1) : : "scc"))
#undef FIN
// ---- readlane (VALU->SGPR) chains
#define FIN out[blockIdx.x * 64 + threadIdx.x] = (unsigned long long)(a0 + s0 + s1 + s2 + s3)
KERNEL(k_readlane, unsigned a0 = threadIdx.x; unsigned s0 = 0; unsigned s1 = 0; unsigned s2 = 0; unsigned s3 = 0,
       asm volatile("v_readlane_b32 %0, %4, 3\n v_readlane_b32 %1, %4, 5\n v_readlane_b32 %2, %4, 7\n v_readlane_b32 %3, %4, 9"
                    : "=s"(s0), "=s"(s1), "=s"(s2), "=s"(s3) : "v"(a0)))
#undef FIN
// ---- LDS read b32 / b64 (independent, no wait inside the group)
#define FIN out[blockIdx.x * 64 + threadIdx.x] = (unsigned long long)(a0 + a1 + a2 + a3)
__global__ __launch_bounds__(64) void k_ldsread(unsigned long long *out, int iters) {
    __shared__ unsigned buf[1024];
    for (int i = threadIdx.x; i < 1024; i += 64) buf[i] = i;
    __syncthreads();
    unsigned a0 = 0, a1 = 0, a2 = 0, a3 = 0;
    unsigned addr = threadIdx.x * 4;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int r = 0; r < REP / 4; ++r) {
            unsigned t0, t1, t2, t3;
            asm volatile("ds_read_b32 %0, %4\n ds_read_b32 %1, %4 offset:256\n ds_read_b32 %2, %4 offset:512\n ds_read_b32 %3, %4 offset:768\n s_waitcnt lgkmcnt(0)"
                         : "=v"(t0), "=v"(t1), "=v"(t2), "=v"(t3) : "v"(addr));
            a0 += t0; a1 += t1; a2 += t2; a3 += t3;
        }
    }
    FIN;
}
// dependent LDS read chain: latency
__global__ __launch_bounds__(64) void k_ldslat(unsigned long long *out, int iters) {
    __shared__ unsigned buf[1024];
    for (int i = threadIdx.x; i < 1024; i += 64) buf[i] = ((i * 7 + 13) & 1023) * 4;
    __syncthreads();
    unsigned addr = threadIdx.x * 4;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int r = 0; r < REP; ++r) {
            asm volatile("ds_read_b32 %0, %0\n s_waitcnt lgkmcnt(0)" : "+v"(addr));
        }
    }
    out[blockIdx.x * 64 + threadIdx.x] = addr;
}
#undef FIN

// ---- branches (SQ_INSTS_BRANCH; not part of SQ_INSTS_SALU): REP back-to-back branches per iteration, all forward and all inside
// one asm statement, SCC set to 0 once per statement (one s_cmp per REP branches).  "+ valu": one independent v_add_u32 behind every
// branch (four registers in turn), reported per (branch, v_add) pair.  The far form skips 32 dwords (128 bytes, two
// instruction-cache lines of 64 bytes) per branch.
#define REP_DIV4 16
#define BR_STR_(x) #x
#define BR_STR(x) BR_STR_(x)
static_assert(REP_DIV4 * 4 == REP, "the branch kernels repeat four branches REP / 4 times");
#define BR4(one) one one one one
#define BR_NT "s_cbranch_scc1 9f\n"
#define BR_TK "s_cbranch_scc0 1f\n s_nop 0\n 1:\n"
#define BR_UN "s_branch 1f\n s_nop 0\n 1:\n"
#define BR_FAR "s_cbranch_scc0 1f\n .rept 32\n s_nop 0\n .endr\n 1:\n"
#define BRANCH_KERNEL(name, one)                                                                                    \
    __global__ __launch_bounds__(64) void name(unsigned long long *out, int iters) {                                \
        unsigned a0 = threadIdx.x;                                                                                  \
        for (int it = 0; it < iters; ++it)                                                                          \
            asm volatile("s_cmp_lg_u32 0, 0\n .rept " BR_STR(REP_DIV4) "\n" BR4(one) ".endr\n 9:\n" : "+v"(a0) : : "scc"); \
        out[blockIdx.x * 64 + threadIdx.x] = a0;                                                                    \
    }
#define BRANCH_VALU_KERNEL(name, one)                                                                               \
    __global__ __launch_bounds__(64) void name(unsigned long long *out, int iters) {                                \
        unsigned a0 = threadIdx.x, a1 = 1, a2 = 2, a3 = 3;                                                          \
        for (int it = 0; it < iters; ++it)                                                                          \
            asm volatile("s_cmp_lg_u32 0, 0\n .rept " BR_STR(REP_DIV4) "\n"                                         \
                         one "v_add_u32 %0, %0, %0\n" one "v_add_u32 %1, %1, %1\n"                                  \
                         one "v_add_u32 %2, %2, %2\n" one "v_add_u32 %3, %3, %3\n"                                  \
                         ".endr\n 9:\n" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) : : "scc");                        \
        out[blockIdx.x * 64 + threadIdx.x] = (unsigned long long)(a0 + a1 + a2 + a3);                               \
    }
BRANCH_KERNEL(k_br_nt, BR_NT)
BRANCH_KERNEL(k_br_tk, BR_TK)
BRANCH_KERNEL(k_br_un, BR_UN)
BRANCH_KERNEL(k_br_far, BR_FAR)
BRANCH_VALU_KERNEL(k_brv_nt, BR_NT)
BRANCH_VALU_KERNEL(k_brv_tk, BR_TK)
BRANCH_VALU_KERNEL(k_brv_un, BR_UN)
BRANCH_VALU_KERNEL(k_brv_far, BR_FAR)

// ---- the scalar port: does a branch, an s_nop or an s_waitcnt take the issue slot of an s_add_u32?  Every row below is reported
// per PAIR (REP / 2 pairs per loop trip), so 2 x the s_add_u32 row means one shared slot and 1 x means a port of its own.
// The adds are `s, s, 1` on four registers in turn: no carry, so SCC stays 0 and the s_cbranch_scc1 behind each falls through.
#define PAIR_KERNEL(name, other)                                                                                    \
    __global__ __launch_bounds__(64) void name(unsigned long long *out, int iters) {                                \
        unsigned s0 = blockIdx.x & 1, s1 = 1, s2 = 2, s3 = 3;                                                        \
        for (int it = 0; it < iters; ++it)                                                                          \
            asm volatile(".rept " BR_STR(REP_DIV4) " / 2\n"                                                         \
                         "s_add_u32 %0, %0, 1\n" other "s_add_u32 %1, %1, 1\n" other                                \
                         "s_add_u32 %2, %2, 1\n" other "s_add_u32 %3, %3, 1\n" other                                \
                         ".endr\n 9:\n" : "+s"(s0), "+s"(s1), "+s"(s2), "+s"(s3) : : "scc");                        \
        out[blockIdx.x * 64 + threadIdx.x] = (unsigned long long)(s0 + s1 + s2 + s3);                               \
    }
PAIR_KERNEL(k_pair_add_add, "s_add_u32 %0, %0, 1\n")        // the yardstick: two adds
PAIR_KERNEL(k_pair_add_br, BR_NT)
PAIR_KERNEL(k_pair_add_nop, "s_nop 0\n")
PAIR_KERNEL(k_pair_add_wait, "s_waitcnt lgkmcnt(0)\n")      // nothing is outstanding
// The same pair split across waves: a wave whose slot on its SIMD (HW_ID bits 3:0) is even only adds, an odd one only branches,
// REP instructions per trip each.  Reported per wave-instruction per SIMD like the one-class rows: 4.4 = one shared slot, 2.2 = two
// ports (at an even number of waves).  out[block * 64] keeps (role, HW_ID, XCC_ID) so that main() can print how the roles fell.
__global__ __launch_bounds__(64) void k_split_add_br(unsigned long long *out, int iters) {
    unsigned hw, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)\n s_getreg_b32 %1, hwreg(HW_REG_XCC_ID)" : "=s"(hw), "=s"(xcc));
    const unsigned role = hw & 1u;
    unsigned s0 = blockIdx.x & 1, s1 = 1, s2 = 2, s3 = 3;
    if (role == 0) {
        for (int it = 0; it < iters; ++it)
            asm volatile(".rept " BR_STR(REP_DIV4) "\n s_add_u32 %0, %0, 1\n s_add_u32 %1, %1, 1\n s_add_u32 %2, %2, 1\n s_add_u32 %3, %3, 1\n .endr"
                         : "+s"(s0), "+s"(s1), "+s"(s2), "+s"(s3) : : "scc");
    } else {
        for (int it = 0; it < iters; ++it)
            asm volatile("s_cmp_lg_u32 0, 0\n .rept " BR_STR(REP_DIV4) "\n" BR4(BR_NT) ".endr\n 9:\n" : "+s"(s0) : : "scc");
    }
    out[blockIdx.x * 64 + threadIdx.x] = (unsigned long long)role | ((unsigned long long)(hw & 0xFFFFu) << 8) | ((unsigned long long)(xcc & 0xFu) << 24)
                                         | ((unsigned long long)((s0 + s1 + s2 + s3) & 1u) << 63);
}
// An EXEC-masked operation against a select in the same place: s_and_saveexec_b64 + s_or_b64 exec around a v_add_u32 (standing for
// the store), against v_cndmask_b32 + the v_add_u32; and the same two around a real ds_write_b16 (the interferer list's store: the
// masked lanes store their value, the select form stores from every lane, the non-members to one scratch halfword).
#define FIN out[blockIdx.x * 64 + threadIdx.x] = (unsigned long long)(a0 + a1 + a2 + a3)
#define MASK_DECL unsigned a0 = threadIdx.x, a1 = 1, a2 = 2, a3 = 3; unsigned long long m = 0x5555555555555555ull + (unsigned long long)(iters & 2); unsigned long long sv
KERNEL(k_saveexec, MASK_DECL,
       asm volatile("s_and_saveexec_b64 %4, %5\n v_add_u32 %0, %0, %0\n s_or_b64 exec, exec, %4\n s_and_saveexec_b64 %4, %5\n v_add_u32 %1, %1, %1\n s_or_b64 exec, exec, %4\n"
                    "s_and_saveexec_b64 %4, %5\n v_add_u32 %2, %2, %2\n s_or_b64 exec, exec, %4\n s_and_saveexec_b64 %4, %5\n v_add_u32 %3, %3, %3\n s_or_b64 exec, exec, %4"
                    : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "=&s"(sv) : "s"(m) : "scc"))
KERNEL(k_cndmask, MASK_DECL; (void)sv,
       asm volatile("v_cndmask_b32_e64 %0, %1, %0, %4\n v_add_u32 %0, %0, %0\n v_cndmask_b32_e64 %1, %2, %1, %4\n v_add_u32 %1, %1, %1\n"
                    "v_cndmask_b32_e64 %2, %3, %2, %4\n v_add_u32 %2, %2, %2\n v_cndmask_b32_e64 %3, %0, %3, %4\n v_add_u32 %3, %3, %3"
                    : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) : "s"(m)))
#undef FIN
#define LDS_STORE_KERNEL(name, body)                                                                                \
    __global__ __launch_bounds__(64) void name(unsigned long long *out, int iters) {                                \
        __shared__ unsigned short buf[1024];                                                                         \
        for (int i = threadIdx.x; i < 1024; i += 64) buf[i] = 0;                                                     \
        __syncthreads();                                                                                            \
        const unsigned addr = (unsigned)(uintptr_t)(const __attribute__((address_space(3))) char *)buf + threadIdx.x * 2, spare = addr - threadIdx.x * 2 + 1024; \
        unsigned a0 = threadIdx.x, t = 0; unsigned long long m = 0x5555555555555555ull + (unsigned long long)(iters & 2), sv = 0; \
        for (int it = 0; it < iters; ++it) {                                                                        \
            _Pragma("unroll") for (int r = 0; r < REP / 4; ++r) { body; }                                           \
        }                                                                                                           \
        __syncthreads();                                                                                            \
        out[blockIdx.x * 64 + threadIdx.x] = (unsigned long long)buf[threadIdx.x] + t + (unsigned)sv + spare;       \
    }
LDS_STORE_KERNEL(k_saveexec_ds,
       asm volatile("s_and_saveexec_b64 %0, %1\n ds_write_b16 %2, %3\n s_or_b64 exec, exec, %0\n s_and_saveexec_b64 %0, %1\n ds_write_b16 %2, %3 offset:128\n s_or_b64 exec, exec, %0\n"
                    "s_and_saveexec_b64 %0, %1\n ds_write_b16 %2, %3 offset:256\n s_or_b64 exec, exec, %0\n s_and_saveexec_b64 %0, %1\n ds_write_b16 %2, %3 offset:384\n s_or_b64 exec, exec, %0\n"
                    "s_waitcnt lgkmcnt(0)" : "=&s"(sv) : "s"(m), "v"(addr), "v"(a0) : "scc", "memory"))
LDS_STORE_KERNEL(k_cndmask_ds,
       asm volatile("v_cndmask_b32_e64 %0, %3, %2, %1\n ds_write_b16 %0, %4\n v_cndmask_b32_e64 %0, %3, %2, %1\n ds_write_b16 %0, %4 offset:128\n"
                    "v_cndmask_b32_e64 %0, %3, %2, %1\n ds_write_b16 %0, %4 offset:256\n v_cndmask_b32_e64 %0, %3, %2, %1\n ds_write_b16 %0, %4 offset:384\n"
                    "s_waitcnt lgkmcnt(0)" : "=&v"(t) : "s"(m), "v"(addr), "v"(spare), "v"(a0) : "memory"))

typedef void (*kern_t)(unsigned long long *, int);
struct Entry { const char *name; kern_t k; int insts_per_iter; };

// how the two roles of k_split_add_br fell on the SIMDs: waves that add / waves that branch on a SIMD -> number of such SIMDs
static char split_note[1024];
static void split_roles(const unsigned long long *out, int blocks, int w) {
    std::vector<unsigned long long> h((size_t)blocks * 64);
    hipMemcpy(h.data(), out, h.size() * 8, hipMemcpyDeviceToHost);
    std::vector<unsigned long long> keys;
    for (int b = 0; b < blocks; b++) keys.push_back((((h[(size_t)b * 64] >> 8) & 0xFF30u) | ((h[(size_t)b * 64] >> 24 & 0xFu) << 16)) << 1 | (h[(size_t)b * 64] & 1u));
    std::sort(keys.begin(), keys.end());
    int hist[17][17] = {};
    for (size_t i = 0; i < keys.size();) {
        size_t j = i; int n[2] = {0, 0};
        while (j < keys.size() && (keys[j] >> 1) == (keys[i] >> 1)) n[keys[j++] & 1]++;
        hist[n[0] > 16 ? 16 : n[0]][n[1] > 16 ? 16 : n[1]]++;
        i = j;
    }
    size_t at = strlen(split_note);
    at += snprintf(split_note + at, sizeof split_note - at, "#   %dw/SIMD:", w);
    for (int x = 0; x < 17; x++) for (int y = 0; y < 17; y++)
        if (hist[x][y] && at < sizeof split_note - 40) at += snprintf(split_note + at, sizeof split_note - at, " %d add + %d branch on %d SIMDs;", x, y, hist[x][y]);
    snprintf(split_note + at, sizeof split_note - at, "\n");
}

int main() {
    hipDeviceProp_t prop;
    hipGetDeviceProperties(&prop, 0);
    const int cus = prop.multiProcessorCount;
    unsigned long long *out;
    hipMalloc(&out, (size_t)cus * 64 * 64 * 8);
    Entry es[] = {{"v_add_u32 (4 indep)", k_valu32, REP}, {"v_add_u32 (dependent)", k_valu32_dep, REP}, {"v_lshlrev_b64", k_shl64, REP},
                  {"v_fma_f64", k_fma64, REP}, {"v_add_f64", k_add64f, REP}, {"v_mul_lo_u32", k_mullo, REP}, {"v_mov_b32_dpp", k_dppmov, REP},
                  {"v_alignbit_b32", k_alignbit, REP}, {"s_add_u32", k_salu, REP}, {"mixed v_add/s_add", k_mixed, REP},
                  {"v_readlane_b32", k_readlane, REP}, {"ds_read_b32 x4 + wait", k_ldsread, REP}, {"ds_read_b32 dependent", k_ldslat, REP},
                  {"s_cbranch_scc1 not taken", k_br_nt, REP}, {"s_cbranch_scc0 taken +1", k_br_tk, REP},
                  {"s_branch +1", k_br_un, REP}, {"s_cbranch_scc0 taken +32", k_br_far, REP},
                  {"not taken + valu", k_brv_nt, REP}, {"taken +1 + valu", k_brv_tk, REP},
                  {"s_branch +1 + valu", k_brv_un, REP}, {"taken +32 + valu", k_brv_far, REP},
                  {"pair s_add + s_add", k_pair_add_add, REP / 2}, {"pair s_add + branch n.t.", k_pair_add_br, REP / 2},
                  {"pair s_add + s_nop 0", k_pair_add_nop, REP / 2}, {"pair s_add + s_waitcnt", k_pair_add_wait, REP / 2},
                  {"split waves: add | branch", k_split_add_br, REP},
                  {"saveexec, v_add, or exec", k_saveexec, REP}, {"v_cndmask, v_add", k_cndmask, REP},
                  {"saveexec, ds_write, or", k_saveexec_ds, REP}, {"v_cndmask, ds_write", k_cndmask_ds, REP}};
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    printf("CUs %d; clock reported %d kHz. cycles per wave-instruction PER SIMD at 2.4 GHz (lower = faster); waves/SIMD = blocks per CU / 4\n", cus, prop.clockRate);
    printf("%-26s", "instruction");
    const int wps[] = {1, 2, 4, 5, 8};
    for (int w : wps) printf("  %4dw/SIMD", w);
    printf("\n");
    for (auto &e : es) {
        printf("%-26s", e.name);
        for (int w : wps) {
            const int blocks = cus * 4 * w;   // one wave per block; the dispatcher spreads them over CUs/SIMDs
            hipLaunchKernelGGL(e.k, dim3(blocks), dim3(64), 0, 0, out, 10);
            hipDeviceSynchronize();
            hipEventRecord(e0);
            hipLaunchKernelGGL(e.k, dim3(blocks), dim3(64), 0, 0, out, ITERS);
            hipEventRecord(e1);
            hipEventSynchronize(e1);
            float ms;
            hipEventElapsedTime(&ms, e0, e1);
            // per SIMD: w waves x ITERS x insts ; cycles = ms*2.4e6
            const double cyc = (double)ms * 2.4e6 / ((double)w * ITERS * e.insts_per_iter);
            printf("  %9.2f", cyc);
            if (e.k == k_split_add_br) split_roles(out, blocks, w);
        }
        printf("\n");
    }
    printf("# split waves, roles per SIMD (by HW_ID / XCC_ID):\n%s", split_note);
    return 0;
}
