// --blank-geom: the largest non-blank region of a partly blank tile (reference src/utils.py:482-530, correct_partly_blank_geom), from the
// decoded uint8 RGB images of a batch while they lie in HBM.  Per examined frame:
//   m = max(R, G, B) < 250 (the mask blank_stats.hip counts as nonblank_px);
//   the 8-connected components of m and the 4-connected regions of ~m, every region that touches the frame's border being part of one
//   "outside" region; a label is the row-major index of the component's first pixel (outside: -1), so it does not depend on scheduling;
//   E(C) = sum over the pixels (x, y) of C of (x + 1) [right neighbour is outside] - x [left neighbour is outside]: the area inside C's
//   exterior ring when nothing encloses C, less than its encloser's E otherwise; the winner is arg max E, ties to the smallest label;
//   the winner's pixel count, bounding box and outer edges (unit edges between it and the outside region or the frame's border).
//
// Both labellings live in ONE union-find forest per frame: node 0 is the outside region, node i + 1 is pixel i; a parent is never larger
// than its child, so a root is the smallest node of its set: the first pixel, or the outside.  Foreground pixels are only ever united with
// foreground pixels and background with background (or node 0), so the two families of trees never mix.  Launches of one call, all on the
// caller's stream, a wave taking 64 consecutive pixels of a row at a time (no LDS, no barriers: the waves are independent):
//   init     mask bytes from the image; parent = first pixel of the pixel's run inside its 64-pixel piece (a ballot); E slots and
//            accumulators cleared
//   unite    the links a row scan needs: to the row above (N; NW and NE for the foreground when N is off), across piece borders, and from
//            background pixels on the frame's border to node 0 -- find, then atomicMin on the larger root until both sides agree
//   flatten  parent = root
//   area     E per component with 64-bit integer atomics; a component's slot is that of its first pixel's 2 x 1 cell (two first pixels
//            cannot share one: they would be neighbours)
//   winner   components counted, max over (E << 31 | INT_MAX - label) with a 64-bit atomicMax
//   stats    the winner's pixel count, box, outer edges and edge pixels; the two label maps when asked for
//   record   one aq_blank_geom per frame
// aq_blank_ring_edges_u8 reads the same scratch again and writes (pixel index, side mask) of every winner pixel with an outer edge.
// Only integer atomics whose results do not depend on their order (min, max, add): two calls give the same records.  Unbounded loops: find
// (parents decrease strictly) and unite (the larger of the two roots decreases strictly).
#include "aq_common.h"
#include <limits.h>

namespace {

constexpr int kAcc = 16;   // per frame: examined, n_components, key (2 words), px, x0, y0, x1, y1, n_edges, edge_px, edge cursor, 4 unused
enum { A_EXAMINED = 0, A_NCOMP = 1, A_KEY = 2, A_PX = 4, A_X0 = 5, A_Y0 = 6, A_X1 = 7, A_Y1 = 8, A_NEDGES = 9, A_EDGEPX = 10, A_CURSOR = 11 };

struct GeomParams {
    const unsigned char* img;
    const aq_frame* frames;
    int n_frames;
    const aq_blank_stat* stats;         // or null: every frame is examined
    int* acc;                           // [n_frames][kAcc]
    unsigned long long* area;           // E slots, frame i's from frames[i].mcu / 2
    int* parent;                        // nodes, frame i's from frames[i].mcu
    unsigned char* mask;                // frame i's from frames[i].mcu
    aq_blank_geom* out;
    int* labels;                        // or null
    const long long* edge_at;           // ring edges: [n_frames + 1]
    int* edges;
};

__device__ __forceinline__ int ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int find(const int* parent, int a) {
    for (int q; (q = ld(parent + a)) != a;) a = q;
    return a;
}

__device__ void unite(int* parent, int a, int b) {
    a = find(parent, a);
    b = find(parent, b);
    while (a != b) {
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(parent + a, b);          // a was a root: it hangs under b now; else what it hung under has to meet b
        if (old == a) break;
        a = old;
    }
}

__device__ __forceinline__ bool examined(const GeomParams& p, int fi) {
    if (!p.stats) return true;
    const aq_blank_stat s = p.stats[fi];
    const bool blank = (s.l_min == s.l_max && (s.l_min == 0 || s.l_min == 1 || s.l_min == 255)) || (s.l_min >= 250 && s.l_max >= 250);
    return !blank && s.blank_rows + s.blank_cols > 0 && s.nonblank_px > 0;       // blank.status: partly blank, and something to outline
}

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ unsigned long long wave_max64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned hi = (unsigned)__shfl_xor((int)(v >> 32), o), lo = (unsigned)__shfl_xor((int)(unsigned)v, o);
        const unsigned long long w = ((unsigned long long)hi << 32) | lo;
        v = w > v ? w : v;
    }
    return v;
}

// The frames of a launch: blockIdx.y strides over them, and the grid's waves stride over a frame's pieces (64 pixels of one row).
struct Walk {
    int lane, segs;
    long long unit, units, step;
    __device__ Walk(const aq_frame& f) {
        lane = threadIdx.x & 63;
        segs = (f.w + 63) >> 6;
        units = (long long)f.h * segs;
        unit = blockIdx.x * 4LL + (threadIdx.x >> 6);
        step = gridDim.x * 4LL;
    }
    __device__ bool more() const { return unit < units; }
    __device__ void next() { unit += step; }
    __device__ int y() const { return (int)(unit / segs); }
    __device__ int x() const { return (int)(unit % segs) * 64 + lane; }
};

// true if the pixel at index i (node i + 1) is background of the outside region; valid once the forest is flat
__device__ __forceinline__ bool outside_at(const unsigned char* mask, const int* parent, int i) { return mask[i] == 0 && parent[i + 1] == 0; }

// the sides of pixel (x, y) that are outer edges: 1 N, 2 E, 4 S, 8 W
__device__ __forceinline__ int outer_sides(const aq_frame& f, const unsigned char* mask, const int* parent, int x, int y) {
    const int i = y * f.w + x;
    int s = 0;
    if (y == 0 || outside_at(mask, parent, i - f.w)) s |= 1;
    if (x == f.w - 1 || outside_at(mask, parent, i + 1)) s |= 2;
    if (y == f.h - 1 || outside_at(mask, parent, i + f.w)) s |= 4;
    if (x == 0 || outside_at(mask, parent, i - 1)) s |= 8;
    return s;
}

__global__ __launch_bounds__(256) void geom_init_kernel(const GeomParams p) {
    for (int fi = blockIdx.y; fi < p.n_frames; fi += gridDim.y) {
        const bool ex = examined(p, fi);
        if (blockIdx.x == 0 && threadIdx.x < kAcc) {
            const int k = threadIdx.x;
            p.acc[(long long)fi * kAcc + k] = k == A_EXAMINED ? (ex ? 1 : 0) : (k == A_X0 || k == A_Y0) ? INT_MAX : (k == A_X1 || k == A_Y1) ? -1 : 0;
        }
        if (!ex) continue;
        const aq_frame f = p.frames[fi];
        int* parent = p.parent + f.mcu;
        unsigned char* mask = p.mask + f.mcu;
        unsigned long long* area = p.area + (f.mcu >> 1);
        const long long slots = (long long)f.h * ((f.w + 1) >> 1);
        for (long long i = blockIdx.x * 256LL + threadIdx.x; i < slots; i += gridDim.x * 256LL) area[i] = 0ull;
        if (blockIdx.x == 0 && threadIdx.x == 0) parent[0] = 0;
        for (Walk w(f); w.more(); w.next()) {
            const int x = w.x(), y = w.y();
            const bool in = x < f.w;
            bool m = false;
            if (in) {
                const unsigned char* s = p.img + f.base + (long long)y * f.pitch + 3LL * x;
                m = max((int)s[0], max((int)s[1], (int)s[2])) < 250;
            }
            const unsigned long long bits = __ballot(m);
            if (in) {
                // the nearest lane below this one that is of the other kind ends the run: the run's first pixel is the one after it
                const unsigned long long other = (m ? ~bits : bits) & ((1ull << w.lane) - 1ull);
                const int first = other ? 64 - __clzll((long long)other) : 0;
                const int i = y * f.w + x;
                parent[i + 1] = i + 1 - (w.lane - first);
                mask[i] = m ? 1 : 0;
            }
        }
    }
}

__global__ __launch_bounds__(256) void geom_unite_kernel(const GeomParams p) {
    for (int fi = blockIdx.y; fi < p.n_frames; fi += gridDim.y) {
        if (!examined(p, fi)) continue;
        const aq_frame f = p.frames[fi];
        int* parent = p.parent + f.mcu;
        const unsigned char* mask = p.mask + f.mcu;
        for (Walk w(f); w.more(); w.next()) {
            const int x = w.x(), y = w.y();
            if (x >= f.w) continue;
            const int i = y * f.w + x, node = i + 1;
            const unsigned char m = mask[i];
            const bool west = x > 0 && mask[i - 1] == m;                       // same kind, so already in one set (same run, or united below)
            if (w.lane == 0 && west) unite(parent, node, node - 1);             // runs were cut at the piece's border
            if (y > 0) {
                const bool n = mask[i - f.w] == m, nw = x > 0 && mask[i - f.w - 1] == m;
                if (n) {
                    if (!(west && nw)) unite(parent, node, node - f.w);         // (west and nw: the western neighbour makes this link)
                } else if (m) {                                                 // diagonals count for the foreground only
                    if (nw && !west) unite(parent, node, node - f.w - 1);
                    if (x < f.w - 1 && mask[i - f.w + 1]) unite(parent, node, node - f.w + 1);
                }
            }
            if (!m && (x == 0 || y == 0 || x == f.w - 1 || y == f.h - 1)) unite(parent, node, 0);
        }
    }
}

__global__ __launch_bounds__(256) void geom_flatten_kernel(const GeomParams p) {
    for (int fi = blockIdx.y; fi < p.n_frames; fi += gridDim.y) {
        if (!examined(p, fi)) continue;
        const aq_frame f = p.frames[fi];
        int* parent = p.parent + f.mcu;
        for (Walk w(f); w.more(); w.next()) {
            const int x = w.x(), y = w.y();
            if (x >= f.w) continue;
            const int node = y * f.w + x + 1;
            __hip_atomic_store(parent + node, find(parent, node), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // (still an ancestor for whoever reads it meanwhile)
        }
    }
}

__global__ __launch_bounds__(256) void geom_area_kernel(const GeomParams p) {
    for (int fi = blockIdx.y; fi < p.n_frames; fi += gridDim.y) {
        if (!examined(p, fi)) continue;
        const aq_frame f = p.frames[fi];
        const int* parent = p.parent + f.mcu;
        const unsigned char* mask = p.mask + f.mcu;
        unsigned long long* area = p.area + (f.mcu >> 1);
        const int half = (f.w + 1) >> 1;
        for (Walk w(f); w.more(); w.next()) {
            const int x = w.x(), y = w.y();
            if (x >= f.w) continue;
            const int i = y * f.w + x;
            if (!mask[i]) continue;
            const bool right = x == f.w - 1 || outside_at(mask, parent, i + 1), left = x == 0 || outside_at(mask, parent, i - 1);
            const long long c = (right ? x + 1 : 0) - (left ? x : 0);
            if (c == 0) continue;
            const int first = parent[i + 1] - 1;                               // the component's first pixel
            atomicAdd(area + (long long)(first / f.w) * half + ((first % f.w) >> 1), (unsigned long long)c);
        }
    }
}

__global__ __launch_bounds__(256) void geom_winner_kernel(const GeomParams p) {
    for (int fi = blockIdx.y; fi < p.n_frames; fi += gridDim.y) {
        if (!examined(p, fi)) continue;
        const aq_frame f = p.frames[fi];
        const int* parent = p.parent + f.mcu;
        const unsigned char* mask = p.mask + f.mcu;
        const unsigned long long* area = p.area + (f.mcu >> 1);
        const int half = (f.w + 1) >> 1;
        int n = 0;
        unsigned long long key = 0ull;
        for (Walk w(f); w.more(); w.next()) {
            const int x = w.x(), y = w.y();
            if (x >= f.w) continue;
            const int i = y * f.w + x;
            if (!mask[i] || parent[i + 1] != i + 1) continue;
            ++n;
            const unsigned long long k = (area[(long long)y * half + (x >> 1)] << 31) | (unsigned long long)(INT_MAX - i);
            key = k > key ? k : key;
        }
        n = wave_sum(n);
        key = wave_max64(key);
        if ((threadIdx.x & 63) == 0 && n) {
            atomicAdd(p.acc + (long long)fi * kAcc + A_NCOMP, n);
            atomicMax((unsigned long long*)(p.acc + (long long)fi * kAcc + A_KEY), key);
        }
    }
}

__global__ __launch_bounds__(256) void geom_stats_kernel(const GeomParams p) {
    for (int fi = blockIdx.y; fi < p.n_frames; fi += gridDim.y) {
        if (!examined(p, fi)) continue;
        const aq_frame f = p.frames[fi];
        const int* parent = p.parent + f.mcu;
        const unsigned char* mask = p.mask + f.mcu;
        int* acc = p.acc + (long long)fi * kAcc;
        const unsigned long long key = *(const unsigned long long*)(acc + A_KEY);
        const int win = key ? INT_MAX - (int)(key & 0x7fffffffull) + 1 : -1;    // the winner's root node; none: no node
        int* fg = p.labels ? p.labels + 2LL * f.mcu : nullptr;
        int* bg = fg ? fg + (long long)f.w * f.h : nullptr;
        int px = 0, x0 = INT_MAX, y0 = INT_MAX, x1 = -1, y1 = -1, n_edges = 0, edge_px = 0;
        for (Walk w(f); w.more(); w.next()) {
            const int x = w.x(), y = w.y();
            if (x >= f.w) continue;
            const int i = y * f.w + x, root = parent[i + 1];
            if (fg) {
                fg[i] = mask[i] ? root - 1 : -1;
                bg[i] = mask[i] ? -2 : root - 1;
            }
            if (root != win || !mask[i]) continue;
            const int s = outer_sides(f, mask, parent, x, y);
            ++px;
            x0 = min(x0, x); y0 = min(y0, y); x1 = max(x1, x); y1 = max(y1, y);
            n_edges += __popc(s);
            edge_px += s ? 1 : 0;
        }
        px = wave_sum(px);
        if (px == 0) continue;                                                  // (the same for the whole wave)
        x0 = wave_min(x0); y0 = wave_min(y0); x1 = wave_max(x1); y1 = wave_max(y1);
        n_edges = wave_sum(n_edges); edge_px = wave_sum(edge_px);
        if ((threadIdx.x & 63) == 0) {
            atomicAdd(acc + A_PX, px);
            atomicMin(acc + A_X0, x0); atomicMin(acc + A_Y0, y0); atomicMax(acc + A_X1, x1); atomicMax(acc + A_Y1, y1);
            if (n_edges) { atomicAdd(acc + A_NEDGES, n_edges); atomicAdd(acc + A_EDGEPX, edge_px); }
        }
    }
}

__global__ __launch_bounds__(256) void geom_record_kernel(const GeomParams p) {
    const int fi = blockIdx.x * 256 + threadIdx.x;
    if (fi >= p.n_frames) return;
    const aq_frame f = p.frames[fi];
    const int* a = p.acc + (long long)fi * kAcc;
    const unsigned long long key = *(const unsigned long long*)(a + A_KEY);
    aq_blank_geom r;
    r.examined = a[A_EXAMINED]; r.n_components = a[A_NCOMP];
    r.label = key ? INT_MAX - (int)(key & 0x7fffffffull) : -1;
    r.px = a[A_PX]; r.area_px = (int)(key >> 31);
    const bool any = key != 0ull;                            // no component (or a skipped frame): the empty box (w, h, -1, -1)
    r.x0 = any ? a[A_X0] : f.w; r.y0 = any ? a[A_Y0] : f.h; r.x1 = any ? a[A_X1] : -1; r.y1 = any ? a[A_Y1] : -1;
    r.n_edges = a[A_NEDGES]; r.edge_px = a[A_EDGEPX]; r.reserved = 0;
    p.out[fi] = r;
}

__global__ __launch_bounds__(256) void geom_cursor_kernel(const GeomParams p) {
    const int fi = blockIdx.x * 256 + threadIdx.x;
    if (fi < p.n_frames) p.acc[(long long)fi * kAcc + A_CURSOR] = 0;
}

__global__ __launch_bounds__(256) void geom_edges_kernel(const GeomParams p) {
    for (int fi = blockIdx.y; fi < p.n_frames; fi += gridDim.y) {
        const aq_blank_geom r = p.out[fi];
        if (!r.examined || r.label < 0) continue;
        const aq_frame f = p.frames[fi];
        if (r.label >= f.w * f.h) continue;
        const int* parent = p.parent + f.mcu;
        const unsigned char* mask = p.mask + f.mcu;
        int* cursor = p.acc + (long long)fi * kAcc + A_CURSOR;
        const long long at = p.edge_at[fi], room = p.edge_at[fi + 1] - at;
        for (Walk w(f); w.more(); w.next()) {
            const int x = w.x(), y = w.y();
            int s = 0;
            const int i = y * f.w + x;
            if (x < f.w && mask[i] && parent[i + 1] == r.label + 1) s = outer_sides(f, mask, parent, x, y);
            const unsigned long long has = __ballot(s != 0);
            if (!has) continue;
            int first = 0;
            if (w.lane == 0) first = atomicAdd(cursor, __popcll(has));
            first = __shfl(first, 0);
            const long long k = first + __popcll(has & ((1ull << w.lane) - 1ull));
            if (s && k < room) {                                                // (a slice sized from the record's edge_px holds them all)
                p.edges[2 * (at + k)] = i;
                p.edges[2 * (at + k) + 1] = s;
            }
        }
    }
}

// Slots of a frame in the scratch: one per node and row end, a multiple of 4 so that every frame's part of every array stays aligned.
long long frame_slots(const aq_frame& f) { return (((long long)f.w + 1) * f.h + 2 + 3) & ~3LL; }

// The table's checks, shared by the entry points: slots of the frames, or -1 with the error set.
long long check_frames(const aq_frame* frames_host, int n_frames, long long image_bytes, bool check_window) {
    long long slots = 0;
    for (int i = 0; i < n_frames; ++i) {
        const aq_frame& f = frames_host[i];
        if (!(f.w > 0 && f.h > 0 && f.w <= 65535 && f.h <= 65535 && (long long)f.w * f.h < INT_MAX && f.base >= 0 && f.pitch >= 3LL * f.w)) {
            aq_set_error("blank_geom: frame %d (%d x %d, pitch %d, at byte %lld) is empty, too large or narrower than its pitch", i, f.w, f.h, f.pitch,
                         (long long)f.base);
            return -1;
        }
        if (check_window && image_bytes >= 0 && f.base + (long long)(f.h - 1) * f.pitch + 3LL * f.w > image_bytes) {
            aq_set_error("blank_geom: frame %d (%d x %d, pitch %d, at byte %lld) leaves its buffer of %lld bytes", i, f.w, f.h, f.pitch,
                         (long long)f.base, image_bytes);
            return -1;
        }
        if (check_window && f.mcu != slots) {
            aq_set_error("blank_geom: frame %d has its scratch at slot %d, not where frame %d's ends (%lld)", i, f.mcu, i - 1, slots);
            return -1;
        }
        slots += frame_slots(f);
        if (slots > INT_MAX) {
            aq_set_error("blank_geom: more than 2^31 scratch slots in one call (examine the frames in smaller groups)");
            return -1;
        }
    }
    return slots;
}

size_t scratch_need(int n_frames, long long slots) { return (size_t)n_frames * kAcc * 4 + (size_t)slots * 9; }

void set_arrays(GeomParams& p, void* scratch_dev, int n_frames, long long slots) {
    p.acc = (int*)scratch_dev;
    p.area = (unsigned long long*)(p.acc + (size_t)n_frames * kAcc);
    p.parent = (int*)(p.area + (size_t)slots / 2);
    p.mask = (unsigned char*)(p.parent + (size_t)slots);
}

dim3 sweep_grid(const aq_frame* frames_host, int n_frames, int cus) {
    long long most = 1;
    for (int i = 0; i < n_frames; ++i) {
        const long long units = (long long)frames_host[i].h * ((frames_host[i].w + 63) >> 6);
        most = units > most ? units : most;
    }
    const unsigned gy = (unsigned)min(n_frames, 1024);
    const long long blocks = (most + 3) / 4, cap = max(1, 32 * cus / (int)gy);
    return dim3((unsigned)(blocks < cap ? blocks : cap), gy);
}

}  // namespace

// Bytes of scratch the two calls need for these frames: 64 per frame and 9 per slot, a frame taking (w + 1) h + 2 slots rounded up to a
// multiple of 4; 0 for no frames or a table the calls would refuse.
extern "C" size_t aq_blank_geom_scratch_bytes(const aq_frame* frames_host, int n_frames) {
    if (!frames_host || n_frames <= 0) return 0;
    const long long slots = check_frames(frames_host, n_frames, 0, false);
    return slots < 0 ? 0 : scratch_need(n_frames, slots);
}

extern "C" int aq_blank_components_u8(const uint8_t* images_dev, long long image_bytes, const aq_frame* frames_dev, const aq_frame* frames_host,
                                      int n_frames, const aq_blank_stat* stats_dev, void* scratch_dev, size_t scratch_bytes,
                                      aq_blank_geom* records_dev, int32_t* labels_out_dev, void* stream) {
    AQ_REQUIRE(n_frames >= 0, "blank_geom: bad number of frames (%d)", n_frames);
    if (n_frames == 0) return AQ_OK;
    AQ_REQUIRE(images_dev && frames_dev && frames_host && scratch_dev && records_dev && image_bytes > 0, "blank_geom: null pointer");
    AQ_REQUIRE(((uintptr_t)frames_dev & 7) == 0 && ((uintptr_t)scratch_dev & 7) == 0 && ((uintptr_t)records_dev & 3) == 0 &&
               ((uintptr_t)stats_dev & 3) == 0 && ((uintptr_t)labels_out_dev & 3) == 0, "blank_geom: unaligned table");
    const long long slots = check_frames(frames_host, n_frames, image_bytes, true);
    if (slots < 0) return AQ_ERR_INVALID;
    const size_t need = scratch_need(n_frames, slots);
    AQ_REQUIRE(scratch_bytes >= need, "blank_geom: %zu bytes of scratch, %zu needed (aq_blank_geom_scratch_bytes)", scratch_bytes, need);
    int cus = 0;
    AQ_CHECK_HIP(aq_cus(&cus));
    GeomParams p = {};
    p.img = images_dev; p.frames = frames_dev; p.n_frames = n_frames; p.stats = stats_dev; p.out = records_dev; p.labels = labels_out_dev;
    set_arrays(p, scratch_dev, n_frames, slots);
    const dim3 grid = sweep_grid(frames_host, n_frames, cus);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(geom_init_kernel, grid, dim3(256), 0, s, p);
    AQ_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(geom_unite_kernel, grid, dim3(256), 0, s, p);
    AQ_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(geom_flatten_kernel, grid, dim3(256), 0, s, p);
    AQ_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(geom_area_kernel, grid, dim3(256), 0, s, p);
    AQ_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(geom_winner_kernel, grid, dim3(256), 0, s, p);
    AQ_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(geom_stats_kernel, grid, dim3(256), 0, s, p);
    AQ_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(geom_record_kernel, dim3((unsigned)((n_frames + 255) / 256)), dim3(256), 0, s, p);
    AQ_CHECK_HIP(hipGetLastError());
    return AQ_OK;
}

extern "C" int aq_blank_ring_edges_u8(const aq_frame* frames_dev, const aq_frame* frames_host, int n_frames, const void* scratch_dev,
                                      size_t scratch_bytes, const aq_blank_geom* records_dev, const long long* edge_at_dev,
                                      const long long* edge_at_host, int32_t* edges_dev, long long edges_room, void* stream) {
    AQ_REQUIRE(n_frames >= 0, "blank_geom: bad number of frames (%d)", n_frames);
    if (n_frames == 0) return AQ_OK;
    AQ_REQUIRE(frames_dev && frames_host && scratch_dev && records_dev && edge_at_dev && edge_at_host && edges_room >= 0, "blank_geom: null pointer");
    AQ_REQUIRE(((uintptr_t)frames_dev & 7) == 0 && ((uintptr_t)scratch_dev & 7) == 0 && ((uintptr_t)records_dev & 3) == 0 &&
               ((uintptr_t)edge_at_dev & 7) == 0 && ((uintptr_t)edges_dev & 3) == 0, "blank_geom: unaligned table");
    const long long slots = check_frames(frames_host, n_frames, -1, true);
    if (slots < 0) return AQ_ERR_INVALID;
    const size_t need = scratch_need(n_frames, slots);
    AQ_REQUIRE(scratch_bytes >= need, "blank_geom: %zu bytes of scratch, %zu needed (aq_blank_geom_scratch_bytes)", scratch_bytes, need);
    AQ_REQUIRE(edge_at_host[0] == 0, "blank_geom: the first frame's edges do not start at 0");
    for (int i = 0; i < n_frames; ++i)
        AQ_REQUIRE(edge_at_host[i + 1] >= edge_at_host[i], "blank_geom: frame %d's edges end before they start", i);
    AQ_REQUIRE(edge_at_host[n_frames] <= edges_room && (edges_dev || edge_at_host[n_frames] == 0),
               "blank_geom: %lld edge pixels, room for %lld", edge_at_host[n_frames], edges_room);
    if (edge_at_host[n_frames] == 0) return AQ_OK;
    int cus = 0;
    AQ_CHECK_HIP(aq_cus(&cus));
    GeomParams p = {};
    p.frames = frames_dev; p.n_frames = n_frames; p.out = const_cast<aq_blank_geom*>(records_dev); p.edge_at = edge_at_dev; p.edges = edges_dev;
    set_arrays(p, const_cast<void*>(scratch_dev), n_frames, slots);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(geom_cursor_kernel, dim3((unsigned)((n_frames + 255) / 256)), dim3(256), 0, s, p);
    AQ_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(geom_edges_kernel, sweep_grid(frames_host, n_frames, cus), dim3(256), 0, s, p);
    AQ_CHECK_HIP(hipGetLastError());
    return AQ_OK;
}
