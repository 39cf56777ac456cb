// ongym_state.hpp — save, restore and fork whole replica states on device (ongym_state_save / _load / ongym_fork,
// include/ongym.h).
//
// Between launches a replica's state is a fixed set of per-replica contiguous blocks in HBM (the mutable arrays of Params:
// occ, svc_a, svc_b, svc_r, DevEnv, plus svc_q, svc_o, move_log, move_n when track_ids), in the layout every kernel stores:
// the lean kernels' M64 record codec is turned back into it at store time.  So one copy mechanism serves every kernel.
//
// Blob: a StateHeader (256 bytes), then `count` replica blocks of block_bytes each; inside a block the sections follow each
// other in the order of StateSection, each rounded up to 16 bytes, so every section of every block starts 16-byte aligned.
//
// Copy kernel: one workgroup of kStateThreads per replica block, pure memory traffic.  The block is a flat list of items
// (16-byte units where a section's per-replica size allows it, else 8- or 4-byte units; DevEnv always in 8-byte words);
// every thread loads up to kStateUnroll items before it stores any, so each workgroup keeps that many loads in flight.
// The DevEnv words the destination keeps (the work counters, and with the flags the stream key or the parameters) are read
// from the destination's current DevEnv by the same thread that writes the word, and merged in registers before the store.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "ongym_device.hpp"

namespace ongym {

enum StateSection { kSecOcc = 0, kSecSvcA, kSecSvcB, kSecSvcR, kSecSvcQ, kSecSvcO, kSecMoveLog, kSecMoveN, kSecEnv, kStateSections };

constexpr uint32_t kStateFormat = 1;
constexpr int kStateThreads = 256;
constexpr int kStateUnroll = 4;
constexpr int kEnvWords = (int)(sizeof(DevEnv) / 8);
static_assert(sizeof(DevEnv) % 8 == 0, "DevEnv is copied in 8-byte words");
static_assert(kEnvWords <= 128, "the kept-word mask of DevEnv has 128 bits");

// the blob's header: written by the pack kernel, read on the host by ongym_state_load
struct StateHeader {
    char magic[8];             // "ONGYMST\0"
    uint32_t format;           // kStateFormat
    uint32_t header_bytes;     // sizeof(StateHeader)
    uint64_t fingerprint;      // of the environment's configuration (state_fingerprint)
    int64_t count;             // replica blocks that follow
    int64_t block_bytes;       // bytes per replica block (multiple of 16)
    int32_t rec32, track_ids, row_words, n_links, capacity, devenv_bytes, n_sections;
    int32_t trace_used;        // the source ran a trace the lean kernels cannot replay: its records may exceed the lean codec
    int32_t req_mode;          // the source's request source (kReqNone / kReqRng / kReqTrace)
    int32_t pad_;
    int64_t sec_bytes[kStateSections];   // per-replica bytes of each section (0: absent)
    int64_t sec_off[kStateSections];     // offset of each section inside a block
    uint64_t reserved_[4];
};
static_assert(sizeof(StateHeader) == 256, "StateHeader is 256 bytes");

// per-section array bases of one set of state arrays (replica r's block of section s at base[s] + r * sec_bytes[s])
struct StateArrays { unsigned char *base[kStateSections]; };

struct StateLayout {
    int64_t bytes[kStateSections];
    int64_t off[kStateSections];
    int32_t shift[kStateSections];       // log2 of the access unit (2, 3 or 4)
    int32_t prefix[kStateSections + 1];  // items before section s; prefix[kStateSections] = items per block
    int64_t block_bytes;
};

enum { kCopyPack = 0, kCopyUnpack = 1, kCopyGather = 2 };

struct StateCopyArgs {
    StateLayout L;
    StateArrays cur;          // the environment's state arrays (pack: source, unpack: destination, gather: source)
    StateArrays alt;          // gather only: the destination set
    unsigned char *blob;      // pack / unpack: the first replica block (behind the header)
    unsigned char *hdr_out;   // pack: where block 0 writes `hdr` (nullptr: no header)
    const int32_t *list;      // pack / unpack: replica of block k (nullptr: k); gather: source of replica k (nullptr: k)
    int32_t batch;
    uint64_t keep_lo, keep_hi;   // DevEnv words (bit w: word w) the destination keeps (unpack, gather)
    StateHeader hdr;
};

__device__ __forceinline__ uint4 state_ld(const unsigned char *p, int shift) {
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (shift == 4) v = *reinterpret_cast<const uint4 *>(p);
    else if (shift == 3) { const uint2 w = *reinterpret_cast<const uint2 *>(p); v.x = w.x; v.y = w.y; }
    else v.x = *reinterpret_cast<const uint32_t *>(p);
    return v;
}

__device__ __forceinline__ void state_st(unsigned char *p, int shift, uint4 v) {
    if (shift == 4) *reinterpret_cast<uint4 *>(p) = v;
    else if (shift == 3) *reinterpret_cast<uint2 *>(p) = make_uint2(v.x, v.y);
    else *reinterpret_cast<uint32_t *>(p) = v.x;
}

// grid (blocks), block kStateThreads.  pack: block k = replica list[k] -> blob block k; unpack: blob block k -> replica
// list[k]; gather: replica list[k] of `cur` -> replica k of `alt` (a list entry outside [0, batch) means k itself).
template <int MODE>
__global__ __launch_bounds__(kStateThreads) void k_state_copy(const StateCopyArgs a) {
    const int k = blockIdx.x, t = threadIdx.x;
    int rs = k, rd = k;
    if (MODE == kCopyPack) rs = a.list ? a.list[k] : k;
    if (MODE == kCopyUnpack) rd = a.list ? a.list[k] : k;
    if (MODE == kCopyGather && a.list) {
        const int s = a.list[k];
        rs = (s < 0 || s >= a.batch) ? k : s;
    }
    if (MODE == kCopyPack && k == 0 && a.hdr_out && t < (int)(sizeof(StateHeader) / 8))
        reinterpret_cast<uint64_t *>(a.hdr_out)[t] = reinterpret_cast<const uint64_t *>(&a.hdr)[t];
    const int total = a.L.prefix[kStateSections];
    for (int i0 = t; i0 < total; i0 += kStateThreads * kStateUnroll) {
        uint4 v[kStateUnroll];
        unsigned char *dst[kStateUnroll];
        int sh[kStateUnroll];
#pragma unroll
        for (int u = 0; u < kStateUnroll; u++) {
            const int i = i0 + u * kStateThreads;
            dst[u] = nullptr;
            sh[u] = 2;
            if (i < total) {
                int s = 0;
                while (i >= a.L.prefix[s + 1]) s++;
                const int shift = a.L.shift[s];
                const size_t byte = (size_t)(i - a.L.prefix[s]) << shift;
                const unsigned char *src;
                if (MODE == kCopyUnpack) src = a.blob + (size_t)k * a.L.block_bytes + a.L.off[s] + byte;
                else src = a.cur.base[s] + (size_t)rs * a.L.bytes[s] + byte;
                if (MODE == kCopyPack) dst[u] = a.blob + (size_t)k * a.L.block_bytes + a.L.off[s] + byte;
                else if (MODE == kCopyUnpack) dst[u] = a.cur.base[s] + (size_t)rd * a.L.bytes[s] + byte;
                else dst[u] = a.alt.base[s] + (size_t)rd * a.L.bytes[s] + byte;
                bool keep = false;
                if (MODE != kCopyPack && s == kSecEnv) {
                    const int w = (int)(byte >> 3);
                    keep = ((w < 64 ? a.keep_lo >> w : a.keep_hi >> (w - 64)) & 1ull) != 0;
                }
                // a kept DevEnv word: the destination's own value (unpack: the word about to be overwritten; gather: the
                // destination replica's word in `cur`)
                if (keep) src = a.cur.base[s] + (size_t)rd * a.L.bytes[s] + byte;
                v[u] = state_ld(src, shift);
                sh[u] = shift;
            }
        }
#pragma unroll
        for (int u = 0; u < kStateUnroll; u++)
            if (dst[u]) state_st(dst[u], sh[u], v[u]);
    }
}

}  // namespace ongym
