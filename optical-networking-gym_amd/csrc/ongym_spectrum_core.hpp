// ongym_spectrum_core.hpp — the two steps of ongym_spectrum_map (include/ongym.h) that decide which addresses the kernel may
// form: decoding and validating a stored service record, and turning a slot range into the mask of one 64-slot row word.
// Plain C++ without any HIP dependency: k_spectrum_map (ongym_spectrum.hpp) and a host program under the sanitizers
// (tests/spectrum_core_main.cpp) compile the same text.
//
// The call is defined on any bytes ongym_state_load accepts, so nothing here indexes a table, and every shift count is
// checked where it is formed.  What passes spectrum_fields_ok satisfies 0 <= slot < slot + n <= S <= 1023, 0 <= path < n_paths
// and 0 <= mod < n_mods, so the claimed cells [slot, min(slot + n + 1, S)) lie inside a row.
#pragma once
#include <stdint.h>

#include "../../include/ongym.h"

#ifdef __HIPCC__
#define ONGYM_SPECTRUM_HD __host__ __device__ inline
#else
#define ONGYM_SPECTRUM_HD inline
#endif

namespace ongym {

constexpr int kSpectrumAudit = ONGYM_N_SPECTRUM_AUDIT_COLUMNS;   // audit_out entries per replica
constexpr int kSpectrumRec = ONGYM_N_SPECTRUM_RECORD_COLUMNS;    // rec_out entries per record
constexpr int kSpectrumMaxOwners = ONGYM_MAX_OWNER_CAPACITY;     // owner_out: a guard cell of record i reads -2 - i >= -32767
constexpr int kOwnerFree = ONGYM_OWNER_FREE, kOwnerUnowned = ONGYM_OWNER_UNOWNED;

struct SpectrumRec { int path, slot, n, mod; };

// The record codecs of ongym_device.hpp (rec_pack), field by field; every field is unsigned, so none is negative.
//   generic : a = path | slot << 16                 b = n | mod << 16   (mod: 8 bits)
//   R32     : a = low word of the route's link mask b = slot | n << 10 | mod << 20 | path << 23
ONGYM_SPECTRUM_HD SpectrumRec spectrum_decode(bool r32, uint32_t a, uint32_t b) {
    SpectrumRec r;
    if (r32) {
        r.path = (int)(b >> 23); r.slot = (int)(b & 0x3FFu); r.n = (int)((b >> 10) & 0x3FFu); r.mod = (int)((b >> 20) & 0x7u);
    } else {
        r.path = (int)(a & 0xFFFFu); r.slot = (int)(a >> 16); r.n = (int)(b & 0xFFFFu); r.mod = (int)((b >> 16) & 0xFFu);
    }
    return r;
}

// Well-formed but for the R32 mask word, which needs the route's mask (looked up only after this has passed).
ONGYM_SPECTRUM_HD bool spectrum_fields_ok(const SpectrumRec &r, int n_paths, int n_mods, int n_slots) {
    return r.path >= 0 && r.path < n_paths && r.n >= 1 && r.slot >= 0 && r.slot + r.n <= n_slots && r.mod >= 0 && r.mod < n_mods;
}

// R32 keeps the low word of the route's link mask in the record: it must be the table's.
ONGYM_SPECTRUM_HD bool spectrum_mask_ok(bool r32, uint32_t a, uint64_t route_mask0) { return !r32 || a == (uint32_t)route_mask0; }

// A = st.active clamped to [0, C]
ONGYM_SPECTRUM_HD int spectrum_active(int active, int capacity) { return active < 0 ? 0 : active > capacity ? capacity : active; }

// One past the last claimed cell of a well-formed record: the guard cell slot + n unless the signal ends at S.
ONGYM_SPECTRUM_HD int spectrum_claim_end(const SpectrumRec &r, int n_slots) { return r.slot + r.n < n_slots ? r.slot + r.n + 1 : r.slot + r.n; }

// Bits [lo, hi) (slot coordinates of the row) that fall into row word w; any lo, hi, w.
ONGYM_SPECTRUM_HD uint64_t spectrum_word_mask(int w, int lo, int hi) {
    const long long base = 64ll * w;
    const long long a = lo > base ? lo - base : 0, b = hi - base < 64 ? hi - base : 64;
    if (b <= a) return 0;                         // then 0 <= a < b <= 64
    const uint64_t m = (b - a == 64) ? ~0ull : ((1ull << (b - a)) - 1ull);
    return m << a;                                // a <= 63
}

}  // namespace ongym
