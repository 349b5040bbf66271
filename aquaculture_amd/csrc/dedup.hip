// --dedup-years: one year's cages per tile and image pass (reference src/utils_tonnage.py:668-911, dedup_cages_in_overlap_years_with_white_space).
// The images of one (pass, tile key) group share a pixel grid; every image that takes part is a slot with a mask: the whole frame (FULL) or
// the even-odd fill of its exterior pixel ring (BITMAP).  The reference allots slot i, under an order of the slots, its mask minus the masks
// before it, and keeps a cage of slot i iff its box meets that region.  Here the pixels are read once for all n! orders:
//   fill     rings (closed walks of pixel corners, axis-parallel) -> per ring a bitmap of h rows x ceil((w + 1) / 32) words the caller zeroed.
//            Launch 1, one lane per vertex: the segment to the next vertex of the same ring, if vertical at x, toggles bit x of every row it
//            spans (atomicXor; x = w lands in the extra column).  Launch 2, one lane per row: an inclusive prefix XOR over the row's bits
//            (shift-XOR inside a word, the parity carried across words): bit c = an odd number of unit edges of row r at x <= c.
//   sets     one wavefront per cage.  Window: columns max(xmin - 1, 0) .. min(xmax, w - 1), rows max(ymin - 1, 0) .. min(ymax, h - 1) (a closed
//            box meets a closed pixel square when it touches it).  Lanes stride over the (row, word column) positions of the window, load the
//            n mask words (FULL: all ones), keep the window's columns, and for every slot set S that holds the cage's slot i test
//            AND(w_j, j in S) & AND(~w_j, j not in S) != 0.  Bit S of the cage's uint32 word = some pixel of the window lies in exactly the
//            masks of S.  A slot outside [0, n), an ABSENT slot, a group outside [0, G) or an empty window give 0.
//   select   one wavefront per group, lanes over the n! orders (itertools.permutations(range(n)) order, so two rounds for n = 5).  A cage of
//            slot i survives an order iff its word has a set S without any slot that comes before i.  Each lane adds the areas (NaN counts
//            as 0) of its order's survivors, one cage at a time in ascending cage position, from +0.0; then lane 0 walks the n! sums in
//            order: max = the last order whose sum is >= the running best (from 0), min = the first whose sum is < the running best (from
//            +inf); random = the order the host gives.  An order that is never chosen is -1 and keeps no cage.  Per cage the bits
//            AQ_DEDUP_SEL_MIN | _MAX | _RANDOM of the selections it survives.
// Integer atomics only, fp64 + only, no allocation: two calls give the same bytes.  Every index is kept inside its array on the device.
#include "aq_common.h"

namespace {

constexpr int kSlots = (int)sg::kDedupMaxSlots, kPerms = (int)sg::kDedupMaxPerms;
static_assert(kSlots == AQ_DEDUP_MAX_SLOTS && kPerms == AQ_DEDUP_MAX_PERMS && kSlots == 5 && kPerms == 120, "dedup: the header's limits");

struct FillParams {
    const int* ring_xy;        // [V][2]
    const int* ring_start;     // [R + 1]
    const int* ring_frame;     // [R][4]: first bitmap word, w, h, reserved
    unsigned* bitmap;          // [bitmap_words]
    long long V, R, bitmap_words;
};

// ring r's frame kept inside the bitmap: false if it does not fit
__device__ __forceinline__ bool frame_of(const int* f, long long bitmap_words, long long* word0, int* w, int* h, int* pitch) {
    const int4 v = *(const int4*)f;
    *word0 = v.x; *w = v.y; *h = v.z;
    if (v.y < 1 || v.z < 1 || v.y > (int)sg::kDedupMaxSide || v.z > (int)sg::kDedupMaxSide || v.x < 0) return false;
    *pitch = (v.y + 32) >> 5;                                                   // ceil((w + 1) / 32)
    return (long long)v.x + (long long)v.z * *pitch <= bitmap_words;
}

__global__ __launch_bounds__(256) void dedup_toggle_kernel(const FillParams p) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;              // one lane per vertex: the segment v -> v + 1
    if (v >= p.V) return;
    long long lo = 0, hi = p.R;                                                 // the last ring with ring_start[r] <= v
    while (hi - lo > 1) {
        const long long mid = (lo + hi) >> 1;
        if (p.ring_start[mid] <= v) lo = mid; else hi = mid;
    }
    const long long r = lo;
    long long end = p.ring_start[r + 1];
    end = end > p.V ? p.V : end;
    if (p.ring_start[r] > v || v + 1 >= end) return;
    long long word0; int w, h, pitch;
    if (!frame_of(p.ring_frame + 4 * r, p.bitmap_words, &word0, &w, &h, &pitch)) return;
    const int2 a = *(const int2*)(p.ring_xy + 2 * v), b = *(const int2*)(p.ring_xy + 2 * (v + 1));
    if (a.x != b.x || a.x < 0 || a.x > w) return;                               // only vertical segments toggle
    int y0 = a.y < b.y ? a.y : b.y, y1 = a.y < b.y ? b.y : a.y;                 // rows y0 .. y1 - 1
    y0 = y0 < 0 ? 0 : y0; y1 = y1 > h ? h : y1;
    unsigned* col = p.bitmap + word0 + (a.x >> 5);
    const unsigned bit = 1u << (a.x & 31);
    for (int y = y0; y < y1; ++y) atomicXor(col + (long long)y * pitch, bit);
}

__global__ __launch_bounds__(64) void dedup_prefix_kernel(const FillParams p) {
    const long long r = blockIdx.x;                                             // one block per ring, lanes stride over its rows
    long long word0; int w, h, pitch;
    if (!frame_of(p.ring_frame + 4 * r, p.bitmap_words, &word0, &w, &h, &pitch)) return;
    for (int y = threadIdx.x; y < h; y += 64) {
        unsigned* row = p.bitmap + word0 + (long long)y * pitch;
        unsigned carry = 0;
        for (int k = 0; k < pitch; ++k) {
            unsigned t = row[k];
            t ^= t << 1; t ^= t << 2; t ^= t << 4; t ^= t << 8; t ^= t << 16;   // bit c = parity of bits 0 .. c
            t ^= carry;
            carry = 0u - (t >> 31);
            row[k] = t;
        }
    }
}

struct SetsParams {
    const int* group;          // [G][16]: n, w, h, reserved, kind[5], word[5], reserved[2]
    const int* cage;           // [C][8]: group, slot, xmin, xmax, ymin, ymax, reserved[2]
    const unsigned* bitmap;    // [bitmap_words]
    unsigned* words;           // out [C]
    long long G, C, bitmap_words;
};

__global__ __launch_bounds__(64) void dedup_sets_kernel(const SetsParams p) {
    const long long e = blockIdx.x;                                             // one wavefront per cage: everything but `lane` is uniform
    const int lane = threadIdx.x;
    const int4 c0 = *(const int4*)(p.cage + 8 * e), c1 = *(const int4*)(p.cage + 8 * e + 4);
    const int g = c0.x, slot = c0.y;
    unsigned found = 0;
    if (g >= 0 && g < p.G) {
        const int* gt = p.group + 16LL * g;
        int n = gt[0];
        n = n < 0 ? 0 : n > kSlots ? kSlots : n;
        const int w = gt[1], h = gt[2];
        const bool frame_ok = w >= 1 && h >= 1 && w <= (int)sg::kDedupMaxSide && h <= (int)sg::kDedupMaxSide;
        const int pitch = (w + 32) >> 5;
        int kind[kSlots];
        long long off[kSlots];
        for (int j = 0; j < kSlots; ++j) {
            kind[j] = j < n ? gt[4 + j] : AQ_DEDUP_ABSENT;
            off[j] = gt[9 + j];
            // a bitmap that leaves the array counts as empty
            if (kind[j] == AQ_DEDUP_BITMAP && !(frame_ok && off[j] >= 0 && off[j] + (long long)h * pitch <= p.bitmap_words)) kind[j] = AQ_DEDUP_ABSENT;
            if (kind[j] != AQ_DEDUP_BITMAP && kind[j] != AQ_DEDUP_FULL) kind[j] = AQ_DEDUP_ABSENT;
        }
        // xmin - 1 .. xmax and ymin - 1 .. ymax inside the frame (the comparisons come first: no overflow at INT_MIN)
        const int x0 = c0.z <= 0 ? 0 : c0.z - 1, x1 = c0.w > w - 1 ? w - 1 : c0.w;
        const int y0 = c1.x <= 0 ? 0 : c1.x - 1, y1 = c1.y > h - 1 ? h - 1 : c1.y;
        int own = AQ_DEDUP_ABSENT;                                              // (selected, not indexed: the arrays stay in registers)
        for (int j = 0; j < kSlots; ++j) own = slot == j ? kind[j] : own;
        if (frame_ok && own != AQ_DEDUP_ABSENT && x0 <= x1 && y0 <= y1) {
            const int k0 = x0 >> 5, k1 = x1 >> 5, nk = k1 - k0 + 1;
            const long long total = (long long)(y1 - y0 + 1) * nk;
            for (long long i = lane; i < total; i += 64) {
                const int y = y0 + (int)(i / nk), k = k0 + (int)(i % nk);
                const unsigned lo = k == k0 ? (unsigned)(x0 & 31) : 0u, hi = k == k1 ? (unsigned)(x1 & 31) : 31u;
                const unsigned cols = (0xffffffffu >> (31 - hi)) & (0xffffffffu << lo);
                unsigned m[kSlots];
                for (int j = 0; j < kSlots; ++j)
                    m[j] = kind[j] == AQ_DEDUP_FULL ? 0xffffffffu : kind[j] == AQ_DEDUP_BITMAP ? p.bitmap[off[j] + (long long)y * pitch + k] : 0u;
                unsigned mine = 0;
                for (int j = 0; j < kSlots; ++j) mine = slot == j ? m[j] : mine;
                if (!(mine & cols)) continue;
                for (unsigned S = 0; S < (1u << n); ++S) {
                    if (!((S >> slot) & 1)) continue;
                    unsigned t = cols;
                    for (int j = 0; j < kSlots; ++j)
                        if (j < n) t &= ((S >> j) & 1) ? m[j] : ~m[j];
                    if (t) found |= 1u << S;
                }
            }
        }
    }
    for (int s = 32; s >= 1; s >>= 1) found |= __shfl_xor(found, s);
    if (lane == 0) p.words[e] = found;
}

struct SelectParams {
    const int* group;          // [G][16]
    const int* cage_start;     // [G + 1]
    const int* cage;           // [C][8]
    const unsigned* words;     // [C]
    const double* area;        // [C]
    const int* random_order;   // [G][5]
    unsigned char* sel;        // out [C]
    int* chosen;               // out [G][4]: min, max, random, n!
    double* sums;              // out [G][120]
    long long G, C;
};

// position of every slot under order number q of the n! (lexicographic, as itertools.permutations(range(n))); pos[j] = n for j >= n
__device__ __forceinline__ void order_positions(int q, int n, int* pos) {
    const int fact[6] = {1, 1, 2, 6, 24, 120};
    unsigned left = (1u << n) - 1;
    for (int j = 0; j < kSlots; ++j) pos[j] = n;
    for (int k = 0; k < kSlots; ++k) {
        if (k >= n) break;
        const int f = fact[n - 1 - k];
        int d = q / f;
        q -= d * f;
        int j = 0;
        for (int t = 0; t < kSlots; ++t)                                        // the d-th slot still left
            if ((left >> t) & 1) { if (d == 0) { j = t; break; } --d; }
        left &= ~(1u << j);
        pos[j] = k;
    }
}

// for every slot i: the sets S (as bits of a word) that hold no slot placed before i; all zero for q < 0
__device__ __forceinline__ void survivor_masks(const int* pos, int n, bool valid, unsigned* M) {
    for (int i = 0; i < kSlots; ++i) {
        unsigned before = 0;
        for (int j = 0; j < kSlots; ++j) before |= (j < n && pos[j] < pos[i]) ? 1u << j : 0u;
        unsigned mask = 0;
        for (unsigned S = 0; S < 32; ++S) mask |= (S & before) ? 0u : 1u << S;
        M[i] = valid && i < n ? mask : 0u;
    }
}

__global__ __launch_bounds__(64) void dedup_select_kernel(const SelectParams p) {
    __shared__ double s_sum[kPerms];
    __shared__ int s_pick[2];
    const long long g = blockIdx.x;                                             // one wavefront per group
    const int lane = threadIdx.x;
    const int fact[6] = {1, 1, 2, 6, 24, 120};
    int n = p.group[16 * g];
    n = n < 1 ? 1 : n > kSlots ? kSlots : n;
    const int np = fact[n];
    long long first = p.cage_start[g], end = p.cage_start[g + 1];               // kept inside [0, C] whatever the table holds
    first = first < 0 ? 0 : first > p.C ? p.C : first;
    end = end < first ? first : end > p.C ? p.C : end;
    for (int q = lane; q < kPerms; q += 64) {
        double sum = 0.0;
        if (q < np) {
            int pos[kSlots];
            unsigned M[kSlots];
            order_positions(q, n, pos);
            survivor_masks(pos, n, true, M);
            for (long long e = first; e < end; ++e) {
                const int slot = p.cage[8 * e + 1];
                const unsigned wd = p.words[e];
                const double a = p.area[e];
                unsigned m = 0;
                for (int j = 0; j < kSlots; ++j) m = slot == j ? M[j] : m;
                if (wd & m) sum = sum + (a != a ? 0.0 : a);
            }
        }
        s_sum[q] = sum;
        p.sums[kPerms * g + q] = sum;
    }
    __syncthreads();
    if (lane == 0) {
        double best_max = 0.0, best_min = __builtin_inf();
        int qmax = -1, qmin = -1;
        for (int q = 0; q < np; ++q) {
            const double v = s_sum[q];
            if (v >= best_max) { qmax = q; best_max = v; }
            if (v < best_min) { qmin = q; best_min = v; }
        }
        s_pick[0] = qmin; s_pick[1] = qmax;
    }
    __syncthreads();
    const int qmin = s_pick[0], qmax = s_pick[1];
    // the host's order: slot random_order[g][k] is k-th; what is not a slot of the group is skipped, a slot not named comes last
    int rpos[kSlots], pmin[kSlots], pmax[kSlots];
    for (int j = 0; j < kSlots; ++j) rpos[j] = n;
    for (int k = kSlots - 1; k >= 0; --k) {
        const int j = p.random_order[kSlots * g + k];
        for (int t = 0; t < kSlots; ++t) rpos[t] = (t == j && t < n && k < n) ? k : rpos[t];
    }
    unsigned Mr[kSlots], Mn[kSlots], Mx[kSlots];
    survivor_masks(rpos, n, true, Mr);
    order_positions(qmin < 0 ? 0 : qmin, n, pmin);
    survivor_masks(pmin, n, qmin >= 0, Mn);
    order_positions(qmax < 0 ? 0 : qmax, n, pmax);
    survivor_masks(pmax, n, qmax >= 0, Mx);
    for (long long e = first + lane; e < end; e += 64) {
        const int slot = p.cage[8 * e + 1];
        const unsigned wd = p.words[e];
        unsigned mn = 0, mx = 0, mr = 0;
        for (int j = 0; j < kSlots; ++j) { mn = slot == j ? Mn[j] : mn; mx = slot == j ? Mx[j] : mx; mr = slot == j ? Mr[j] : mr; }
        p.sel[e] = (unsigned char)(((wd & mn) ? AQ_DEDUP_SEL_MIN : 0) | ((wd & mx) ? AQ_DEDUP_SEL_MAX : 0) | ((wd & mr) ? AQ_DEDUP_SEL_RANDOM : 0));
    }
    if (lane == 0) {
        // the number of the host's order among the n!: its Lehmer rank (a slot that is not named counts as placed last, ties by slot)
        int rank = 0;
        unsigned left = (1u << n) - 1;
        for (int k = 0; k < n; ++k) {
            int j = 0, best = 0x7fffffff;
            for (int t = 0; t < n; ++t)                                         // the slot still left with the smallest (position, slot)
                if (((left >> t) & 1) && rpos[t] < best) { best = rpos[t]; j = t; }
            rank += __popc(left & ((1u << j) - 1)) * fact[n - 1 - k];
            left &= ~(1u << j);
        }
        *(int4*)(p.chosen + 4 * g) = make_int4(qmin, qmax, rank, np);
    }
}

// the checks on the host copies of the tables that all three launchers share
bool group_table_ok(const int32_t* group_host, long long G, long long bitmap_words, bool need_bitmaps) {
    for (long long g = 0; g < G; ++g) {
        const int32_t* t = group_host + 16 * g;
        if (t[0] < 1 || t[0] > AQ_DEDUP_MAX_SLOTS) {
            aq_set_error("dedup: group %lld has %d images (1 to %d: the longest image pass has %d years)", g, t[0], AQ_DEDUP_MAX_SLOTS, AQ_DEDUP_MAX_SLOTS);
            return false;
        }
        if (!sg::dedup_frame_fits(t[1], t[2])) {
            aq_set_error("dedup: group %lld has a frame of %d x %d pixels (1 to %lld a side)", g, t[1], t[2], sg::kDedupMaxSide);
            return false;
        }
        for (int j = 0; j < t[0]; ++j) {
            const int kind = t[4 + j];
            if (kind != AQ_DEDUP_FULL && kind != AQ_DEDUP_BITMAP && kind != AQ_DEDUP_ABSENT) {
                aq_set_error("dedup: slot %d of group %lld has kind %d", j, g, kind);
                return false;
            }
            if (need_bitmaps && kind == AQ_DEDUP_BITMAP &&
                (t[9 + j] < 0 || (long long)t[9 + j] + (long long)t[2] * sg::dedup_pitch(t[1]) > bitmap_words)) {
                aq_set_error("dedup: the bitmap of slot %d of group %lld ends at word %lld of %lld", j, g,
                             (long long)t[9 + j] + (long long)t[2] * sg::dedup_pitch(t[1]), bitmap_words);
                return false;
            }
        }
    }
    return true;
}

}  // namespace

extern "C" int aq_dedup_fill_u32(const int32_t* ring_xy_dev, long long V, const int32_t* ring_start_dev, const int32_t* ring_start_host,
                                 const int32_t* ring_frame_dev, const int32_t* ring_frame_host, long long R, uint32_t* bitmap_dev,
                                 long long bitmap_words, void* stream) {
    AQ_REQUIRE(sg::dedup_count_fits(V), "dedup: %lld ring vertices (at most 2^31 - 1 in one call)", V);
    AQ_REQUIRE(sg::dedup_count_fits(R), "dedup: %lld rings (at most 2^31 - 1 in one call)", R);
    AQ_REQUIRE(sg::dedup_count_fits(bitmap_words), "dedup: a bitmap of %lld words (at most 2^31 - 1 in one call: fewer groups at a time)", bitmap_words);
    if (R == 0) return AQ_OK;
    AQ_REQUIRE(ring_start_host && ring_frame_host, "dedup: null pointer");
    AQ_REQUIRE(ring_start_host[0] >= 0 && ring_start_host[R] <= V, "dedup: ring_start runs from %d to %d with %lld vertices", ring_start_host[0], ring_start_host[R], V);
    for (long long r = 0; r < R; ++r) {
        const int32_t* f = ring_frame_host + 4 * r;
        AQ_REQUIRE(ring_start_host[r + 1] >= ring_start_host[r], "dedup: ring_start decreases at ring %lld (%d after %d)", r, ring_start_host[r + 1], ring_start_host[r]);
        AQ_REQUIRE(sg::dedup_frame_fits(f[1], f[2]), "dedup: ring %lld has a frame of %d x %d pixels (1 to %lld a side)", r, f[1], f[2], sg::kDedupMaxSide);
        AQ_REQUIRE(f[0] >= 0 && (long long)f[0] + (long long)f[2] * sg::dedup_pitch(f[1]) <= bitmap_words,
                   "dedup: the bitmap of ring %lld (%d rows of %lld words from word %d) does not fit %lld words", r, f[2], sg::dedup_pitch(f[1]), f[0], bitmap_words);
    }
    AQ_REQUIRE(ring_start_dev && ring_frame_dev && bitmap_dev && (V == 0 || ring_xy_dev), "dedup: null pointer");
    AQ_REQUIRE(((uintptr_t)ring_xy_dev & 7) == 0 && ((uintptr_t)ring_start_dev & 3) == 0 && ((uintptr_t)ring_frame_dev & 15) == 0 &&
               ((uintptr_t)bitmap_dev & 3) == 0, "dedup: unaligned array");
    FillParams p = {};
    p.ring_xy = ring_xy_dev; p.ring_start = ring_start_dev; p.ring_frame = ring_frame_dev; p.bitmap = bitmap_dev;
    p.V = V; p.R = R; p.bitmap_words = bitmap_words;
    if (V > 0) {
        hipLaunchKernelGGL(dedup_toggle_kernel, dim3((unsigned)sg::cdiv(V, 256)), dim3(256), 0, (hipStream_t)stream, p);
        AQ_CHECK_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(dedup_prefix_kernel, dim3((unsigned)R), dim3(64), 0, (hipStream_t)stream, p);
    AQ_CHECK_HIP(hipGetLastError());
    return AQ_OK;
}

extern "C" int aq_dedup_sets_u32(const int32_t* group_dev, const int32_t* group_host, long long G, const int32_t* cage_dev, long long C,
                                 const uint32_t* bitmap_dev, long long bitmap_words, uint32_t* words_dev, void* stream) {
    AQ_REQUIRE(sg::dedup_count_fits(G), "dedup: %lld groups (at most 2^31 - 1 in one call)", G);
    AQ_REQUIRE(sg::dedup_count_fits(C), "dedup: %lld cages (at most 2^31 - 1 in one call)", C);
    AQ_REQUIRE(sg::dedup_count_fits(bitmap_words), "dedup: a bitmap of %lld words (at most 2^31 - 1 in one call: fewer groups at a time)", bitmap_words);
    if (C == 0) return AQ_OK;
    AQ_REQUIRE(G == 0 || group_host, "dedup: null pointer");
    if (!group_table_ok(group_host, G, bitmap_words, true)) return AQ_ERR_INVALID;
    AQ_REQUIRE(cage_dev && words_dev && (G == 0 || group_dev) && (bitmap_words == 0 || bitmap_dev), "dedup: null pointer");
    AQ_REQUIRE(((uintptr_t)group_dev & 15) == 0 && ((uintptr_t)cage_dev & 15) == 0 && ((uintptr_t)bitmap_dev & 3) == 0 &&
               ((uintptr_t)words_dev & 3) == 0, "dedup: unaligned array");
    SetsParams p = {};
    p.group = group_dev; p.cage = cage_dev; p.bitmap = bitmap_dev; p.words = words_dev; p.G = G; p.C = C; p.bitmap_words = bitmap_words;
    hipLaunchKernelGGL(dedup_sets_kernel, dim3((unsigned)C), dim3(64), 0, (hipStream_t)stream, p);
    AQ_CHECK_HIP(hipGetLastError());
    return AQ_OK;
}

extern "C" int aq_dedup_select_f64(const int32_t* group_dev, const int32_t* group_host, const int32_t* cage_start_dev,
                                   const int32_t* cage_start_host, long long G, const int32_t* cage_dev, const uint32_t* words_dev,
                                   const double* area_dev, long long C, const int32_t* random_order_dev, uint8_t* sel_dev,
                                   int32_t* chosen_dev, double* sums_dev, void* stream) {
    AQ_REQUIRE(sg::dedup_count_fits(G), "dedup: %lld groups (at most 2^31 - 1 in one call)", G);
    AQ_REQUIRE(sg::dedup_count_fits(C), "dedup: %lld cages (at most 2^31 - 1 in one call)", C);
    if (G == 0) return AQ_OK;
    AQ_REQUIRE(group_host && cage_start_host, "dedup: null pointer");
    if (!group_table_ok(group_host, G, 0, false)) return AQ_ERR_INVALID;
    AQ_REQUIRE(cage_start_host[0] >= 0 && cage_start_host[G] <= C, "dedup: cage_start runs from %d to %d with %lld cages", cage_start_host[0], cage_start_host[G], C);
    for (long long g = 0; g < G; ++g)
        AQ_REQUIRE(cage_start_host[g + 1] >= cage_start_host[g], "dedup: cage_start decreases at group %lld (%d after %d)", g, cage_start_host[g + 1], cage_start_host[g]);
    AQ_REQUIRE(group_dev && cage_start_dev && random_order_dev && chosen_dev && sums_dev && (C == 0 || (cage_dev && words_dev && area_dev && sel_dev)),
               "dedup: null pointer");
    AQ_REQUIRE(((uintptr_t)group_dev & 15) == 0 && ((uintptr_t)cage_dev & 15) == 0 && ((uintptr_t)cage_start_dev & 3) == 0 &&
               ((uintptr_t)words_dev & 3) == 0 && ((uintptr_t)area_dev & 7) == 0 && ((uintptr_t)random_order_dev & 3) == 0 &&
               ((uintptr_t)chosen_dev & 15) == 0 && ((uintptr_t)sums_dev & 7) == 0, "dedup: unaligned array");
    SelectParams p = {};
    p.group = group_dev; p.cage_start = cage_start_dev; p.cage = cage_dev; p.words = words_dev; p.area = area_dev;
    p.random_order = random_order_dev; p.sel = sel_dev; p.chosen = chosen_dev; p.sums = sums_dev; p.G = G; p.C = C;
    hipLaunchKernelGGL(dedup_select_kernel, dim3((unsigned)G), dim3(64), 0, (hipStream_t)stream, p);
    AQ_CHECK_HIP(hipGetLastError());
    return AQ_OK;
}
