// yolov5/val.py: the three device steps behind upstream's mAP table ([UPSTREAM val.py run(), process_batch; utils/metrics.py ap_per_class,
// compute_ap, box_iou]).  Built with -ffp-contract=off: every product, sum and quotient below is rounded once, as written,
// so each output is bit-identical to its numpy restatement in aquaculture_amd/val.py.  Nothing is allocated, everything runs on the caller's
// stream, every store is a plain vector store; the only atomics are integer minima in the matcher and integer maxima and sums in the confusion
// step (vector atomics, all order-free).
//
// aq_val_expand_rows_f32: upstream's multi_label branch of non_max_suppression as rows the existing NMS takes.  pred [B][N][5 + nc] ->
//   rows [B][M][5 + nc]: one row per (source row r, class j) with obj > conf and obj * cls_j > conf (one fp32 product), in (r, j) ascending
//   order -- upstream's .nonzero() order --, carrying the box, obj and cls_j in column 5 + j, zeros in the other class columns.  Three
//   launches: the pairs of an image are cut into chunks of 1024, (1) every chunk counts its passing pairs (a ballot per wavefront), (2) one
//   wavefront per image turns the counts into their exclusive scan -- every chunk's running offset -- and compares the total with M, (3)
//   lane l of a wavefront writes at offset + passing pairs of the wavefronts before it + popcount of the ballot's bits below l.  No atomic
//   append: the order does not depend on scheduling.  Rows count[b] .. M - 1 get obj = 0 (the NMS drops them) and nothing else.  When any
//   image emits more than M rows, launch (3) writes nothing at all; counts hold the true numbers either way.
//
// aq_val_match: process_batch as the closed rule of DESIGN.md section 28, one wavefront (one 64-thread workgroup) per image.  Pass 1: lane
//   l takes the detections l, l + 64, ...; each goes through scale_boxes' inverse letterbox and clip, walks the image's labels (every lane
//   reads the same label: wave-uniform loads) keeping the same-class label of largest IoU, the higher index among equals, and for every
//   threshold it reaches lowers minimum[label][threshold] to its own index.  Pass 2: the same walk again; bit i of a detection is set when
//   the minimum of (its best label, i) is the detection itself.  The minima live in LDS for up to 512 labels, else in the image's slice of
//   the caller's scratch.  Confidence, class and bits are appended at total + the counts of the images before; a one-lane launch then adds
//   the batch's count to total.
//
// aq_val_confusion: [UPSTREAM utils/metrics.py ConfusionMatrix.process_batch] as the closed rule of DESIGN.md section 28, on aq_val_match's
//   inputs, scale_box and label_iou, one wavefront per image.  Pass 1: lane l takes the detections l, l + 64, ...; one with conf above the
//   threshold walks the labels and raises the 64-bit key (iou bits << 32) | detection of its best label of any class -- the largest IoU above
//   the threshold, the higher index among equals -- with an integer atomicMax (IoUs above a positive threshold order as their bit patterns);
//   its best label goes to scratch [B][max_det].  Pass 2: lane l takes the labels l, l + 64, ...: a non-zero key names the detection the label
//   keeps, matrix[its class][label class] += 1, else matrix[nc][label class] += 1.  Pass 3, only when the image has a kept pair: a detection
//   that takes part and is in no label's key adds matrix[its class][nc] += 1.  The keys live in LDS for up to 512 labels, else in the
//   image's slice of the scratch.  The increments are 64-bit integer vector atomics; maxima and sums do not depend on scheduling.
//
// aq_val_scores_f64: ap_per_class after the host's stable sort by (class, -confidence, index).  Every class with labels is a run of the
//   sorted arrays, cut into chunks of 2048 (256 threads x 8 consecutive elements); all launches but the last have one workgroup per (chunk,
//   threshold).  (1) chunk sums of the correct bits, (2) per run an exclusive scan of its chunk sums -- the carried prefix --, (3) tpc = the
//   inclusive integer scan, and the chunk's maximum of precision = tpc / (k + 1), (4) per run the maximum over the later chunks -- the
//   carried suffix --, (5) mpre = the running maximum from the right, (6) per (run, threshold) the 101-point interpolation and the
//   trapezoid sum added in ascending x by one lane, and for threshold 0 the three 1000-point curves.  Integer sums and maxima do not depend
//   on the chunking; the interpolation and the sum are written once, in interp_rule and score_ap_kernel.
#include "aq_common.h"

namespace {

__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}
__device__ __forceinline__ long long wave_sum_i64(long long v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}

// ---------------------------------------------------------------- expand ----------------------------------------------------------------
constexpr int kExpandChunk = 1024;     // (row, class) pairs per workgroup = its threads

struct ExpandParams {
    const float* pred;     // [B][N][no]
    float* rows;           // out [B][M][no]
    int* counts;           // out [B]
    int* chunk_count;      // scratch [B][nchunks]
    int* overflow;         // scratch [1]
    int B, N, nc, no, M, nchunks;
    long long pairs;
    float conf;
};

// whether pair i of image b passes; *row = its source row
__device__ __forceinline__ bool expand_passes(const ExpandParams& p, int b, long long i, const float** row, int* cls) {
    if (i >= p.pairs) return false;
    const int r = (int)(i / p.nc), j = (int)(i - (long long)r * p.nc);
    const float* src = p.pred + ((long long)b * p.N + r) * p.no;
    *row = src;
    *cls = j;
    const float obj = src[4];
    if (!(obj > p.conf)) return false;
    return obj * src[5 + j] > p.conf;
}

__global__ __launch_bounds__(kExpandChunk) void expand_count_kernel(const ExpandParams p) {
    __shared__ int wave_count[kExpandChunk / 64];
    const int b = blockIdx.y, tid = threadIdx.x;
    const float* row; int cls;
    const bool m = expand_passes(p, b, (long long)blockIdx.x * kExpandChunk + tid, &row, &cls);   // (64 bits: the last chunk may end past 2^31)
    const unsigned long long mask = __ballot(m);
    if ((tid & 63) == 0) wave_count[tid >> 6] = __popcll(mask);
    __syncthreads();
    if (tid == 0) {
        int s = 0;
        for (int w = 0; w < kExpandChunk / 64; ++w) s += wave_count[w];
        p.chunk_count[(long long)b * p.nchunks + blockIdx.x] = s;
        if (b == 0 && blockIdx.x == 0) p.overflow[0] = 0;                       // the totals launch sets it
    }
}

// per image, one wavefront (four images per workgroup): the chunk counts become their exclusive scan -- every chunk's running offset --
// and the total goes to counts; an image that emits more than M rows stores 1 into the flag the count launch zeroed
__global__ __launch_bounds__(256) void expand_totals_kernel(const ExpandParams p) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);                          // uniform over the wavefront
    if (b >= p.B) return;
    int* cc = p.chunk_count + (long long)b * p.nchunks;
    int carry = 0;
    for (int base = 0; base < p.nchunks; base += 64) {
        const int c = base + lane;
        const int v = c < p.nchunks ? cc[c] : 0;
        int incl = v;
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const int t = __shfl_up(incl, s, 64);
            if (lane >= s) incl += t;
        }
        if (c < p.nchunks) cc[c] = carry + incl - v;
        carry += __shfl(incl, 63, 64);
    }
    if (lane == 0) {
        p.counts[b] = carry;
        if (carry > p.M) p.overflow[0] = 1;
    }
}

__global__ __launch_bounds__(kExpandChunk) void expand_write_kernel(const ExpandParams p) {
    __shared__ int wave_count[kExpandChunk / 64];
    if (p.overflow[0]) return;                                                  // some image does not fit: nothing is written (uniform)
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int chunk_base = p.chunk_count[(long long)b * p.nchunks + blockIdx.x];   // the running offset the totals launch left here
    const long long i = (long long)blockIdx.x * kExpandChunk + tid;
    const float* row; int cls;
    const bool m = expand_passes(p, b, i, &row, &cls);
    const unsigned long long mask = __ballot(m);
    if (lane == 0) wave_count[wave] = __popcll(mask);
    __syncthreads();
    if (m) {
        int slot = chunk_base + __popcll(mask & ((1ULL << lane) - 1ULL));
        for (int w = 0; w < wave; ++w) slot += wave_count[w];
        if (slot < p.M) {                                                       // (always: the totals launch has compared every count with M)
            float* dst = p.rows + ((long long)b * p.M + slot) * p.no;
            dst[0] = row[0]; dst[1] = row[1]; dst[2] = row[2]; dst[3] = row[3]; dst[4] = row[4];
            for (int k = 0; k < p.nc; ++k) dst[5 + k] = k == cls ? row[5 + k] : 0.0f;
        }
    }
    if (i < p.M && i >= p.counts[b]) p.rows[((long long)b * p.M + i) * p.no + 4] = 0.0f;     // the inert fill: obj = 0, nothing else
}

// ---------------------------------------------------------------- match -----------------------------------------------------------------
constexpr int kMatchLdsLabels = 512;   // labels of one image whose minima fit LDS (20 KB)
constexpr int kNoDet = 0x7fffffff;

struct MatchParams {
    const aq_det* dets;        // [B][max_det], network pixels, descending confidence
    const int* counts;         // [B]
    const float4* lbox;        // [L] label boxes, original pixels
    const int* lcls;           // [L]
    const int* lstart;         // [B + 1]
    const float* geom;         // [B][5]: pad x, pad y, gain, w0, h0
    int* scratch;              // [L][10]
    float* conf_out;           // run-long [cap]
    int* cls_out;
    unsigned short* bits_out;
    long long* total;          // [1]
    long long cap;
    int B, max_det, L;
    float iouv[10];
};

// scale_boxes for one detection: subtract the pad, divide by the gain, clip to the original image (x1, y1, x2, y2 in .x .y .z .w)
__device__ __forceinline__ float4 scale_box(const aq_det& t, float padx, float pady, float gain, float w0, float h0) {
    float4 d;
    d.x = fminf(fmaxf((t.x1 - padx) / gain, 0.0f), w0);
    d.y = fminf(fmaxf((t.y1 - pady) / gain, 0.0f), h0);
    d.z = fminf(fmaxf((t.x2 - padx) / gain, 0.0f), w0);
    d.w = fminf(fmaxf((t.y2 - pady) / gain, 0.0f), h0);
    return d;
}

// box_iou of a label g and a detection d of area area_d = (d.z - d.x) * (d.w - d.y): inter / (area_l + area_d - inter + 1e-7), in that order
__device__ __forceinline__ float label_iou(const float4 g, const float4 d, float area_d) {
    const float area_l = (g.z - g.x) * (g.w - g.y);
    float iw = fminf(g.z, d.z) - fmaxf(g.x, d.x);
    float ih = fminf(g.w, d.w) - fmaxf(g.y, d.y);
    iw = iw > 0.0f ? iw : 0.0f;
    ih = ih > 0.0f ? ih : 0.0f;
    const float inter = iw * ih;
    return inter / (area_l + area_d - inter + 1e-7f);
}

// the detection's best label: same class, largest IoU, the higher index among equal IoUs; -1 without a label of its class
__device__ __forceinline__ int best_label(const MatchParams& p, int ls, int le, const float4 d, int cls, float* best_iou) {
    const float area_d = (d.z - d.x) * (d.w - d.y);
    int best = -1;
    float bi = 0.0f;
    for (int l = ls; l < le; ++l) {
        if (p.lcls[l] != cls) continue;
        const float iou = label_iou(p.lbox[l], d, area_d);
        if (best < 0 || iou >= bi) { best = l; bi = iou; }
    }
    *best_iou = bi;
    return best;
}

__global__ __launch_bounds__(64) void match_kernel(const MatchParams p) {
    __shared__ int lds_min[kMatchLdsLabels * 10];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int cnt = min(max(p.counts[b], 0), p.max_det);
    long long before = 0;
    for (int i = lane; i < b; i += 64) before += min(max(p.counts[i], 0), p.max_det);
    const long long base = p.total[0] + wave_sum_i64(before);
    const int ls = min(max(p.lstart[b], 0), p.L);                               // (a table the caller got wrong stays inside [0, L])
    const int le = min(max(p.lstart[b + 1], ls), p.L);
    const int nl = le - ls;
    int* mins = nl <= kMatchLdsLabels ? lds_min : p.scratch + (long long)ls * 10;
    for (int i = lane; i < nl * 10; i += 64) mins[i] = kNoDet;
    __syncthreads();
    const float padx = p.geom[b * 5 + 0], pady = p.geom[b * 5 + 1], gain = p.geom[b * 5 + 2], w0 = p.geom[b * 5 + 3], h0 = p.geom[b * 5 + 4];
    for (int pass = 0; pass < 2; ++pass) {
        for (int d = lane; d < cnt; d += 64) {
            const aq_det t = p.dets[(long long)b * p.max_det + d];
            const int cls = (int)t.cls;
            float iou;
            const int l = best_label(p, ls, le, scale_box(t, padx, pady, gain, w0, h0), cls, &iou);
            if (pass == 0) {
                if (l >= 0)
                    for (int i = 0; i < 10; ++i)
                        if (iou >= p.iouv[i]) atomicMin(&mins[(l - ls) * 10 + i], d);
            } else {
                unsigned bits = 0;
                if (l >= 0)
                    for (int i = 0; i < 10; ++i)
                        if (iou >= p.iouv[i] && mins[(l - ls) * 10 + i] == d) bits |= 1u << i;
                const long long at = base + d;
                if (at >= 0 && at < p.cap) {
                    p.conf_out[at] = t.conf;
                    p.cls_out[at] = cls;
                    p.bits_out[at] = (unsigned short)bits;
                }
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(64) void match_advance_kernel(const MatchParams p) {
    long long s = 0;
    for (int i = threadIdx.x; i < p.B; i += 64) s += min(max(p.counts[i], 0), p.max_det);
    s = wave_sum_i64(s);
    if (threadIdx.x == 0) p.total[0] += s;
}

// -------------------------------------------------------------- confusion ---------------------------------------------------------------
constexpr int kNotTakingPart = -2;     // best[d] of a detection at or below the confidence threshold; -1 = takes part, no label above the IoU

struct ConfusionParams {
    const aq_det* dets;        // [B][max_det]
    const int* counts;         // [B]
    const float4* lbox;        // [L]
    const int* lcls;           // [L]
    const int* lstart;         // [B + 1]
    const float* geom;         // [B][5]
    unsigned long long* keys;  // scratch [L]: (iou bits << 32) | detection, 0 = no detection
    int* best;                 // scratch [B][max_det]
    unsigned long long* matrix;   // [(nc + 1)][(nc + 1)], [predicted][true]; added to
    int* image;                // out [B][4]
    int* flag;                 // [1]: set to 1 when a class outside [0, nc) is met, never cleared
    int B, max_det, L, nc;
    float conf, iou;
};

__device__ __forceinline__ unsigned long long key_load(const unsigned long long* k) {
    return __hip_atomic_load(k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // (the keys were raised by atomics: read them where those landed)
}

__global__ __launch_bounds__(64) void confusion_kernel(const ConfusionParams p) {
    __shared__ unsigned long long lds_key[kMatchLdsLabels];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int cnt = min(max(p.counts[b], 0), p.max_det);
    const int ls = min(max(p.lstart[b], 0), p.L);
    const int le = min(max(p.lstart[b + 1], ls), p.L);
    const int nl = le - ls;
    unsigned long long* keys = nl <= kMatchLdsLabels ? lds_key : p.keys + ls;
    for (int i = lane; i < nl; i += 64) keys[i] = 0ULL;
    __syncthreads();
    const float padx = p.geom[b * 5 + 0], pady = p.geom[b * 5 + 1], gain = p.geom[b * 5 + 2], w0 = p.geom[b * 5 + 3], h0 = p.geom[b * 5 + 4];
    const aq_det* dets = p.dets + (long long)b * p.max_det;
    int* best = p.best + (long long)b * p.max_det;
    const float ncf = (float)p.nc;
    // pass 1: every detection that takes part finds its best label of any class and raises that label's key
    int part = 0, bad = 0;
    for (int d = lane; d < cnt; d += 64) {
        const aq_det t = dets[d];
        if (!(t.cls >= 0.0f && t.cls < ncf)) bad = 1;
        int l = kNotTakingPart;
        if (t.conf > p.conf) {
            ++part;
            l = -1;
            const float4 box = scale_box(t, padx, pady, gain, w0, h0);
            const float area_d = (box.z - box.x) * (box.w - box.y);
            float bi = 0.0f;
            for (int k = ls; k < le; ++k) {
                const float iou = label_iou(p.lbox[k], box, area_d);
                if (iou > p.iou && iou >= bi) { l = k; bi = iou; }
            }
            if (l >= 0) atomicMax(&keys[l - ls], ((unsigned long long)__float_as_uint(bi) << 32) | (unsigned)d);
        }
        best[d] = l;
    }
    for (int i = lane; i < nl; i += 64) {
        const int gc = p.lcls[ls + i];
        if (gc < 0 || gc >= p.nc) bad = 1;
    }
    part = wave_sum_i32(part);
    bad = wave_sum_i32(bad);
    __syncthreads();
    if (bad) {                                                                  // (uniform) a class outside [0, nc): the image adds nothing
        if (lane == 0) {
            p.flag[0] = 1;
            p.image[b * 4 + 0] = nl; p.image[b * 4 + 1] = 0; p.image[b * 4 + 2] = 0; p.image[b * 4 + 3] = 0;
        }
        return;
    }
    // pass 2: every label's kept detection and its matrix entry
    const long long n1 = (long long)p.nc + 1;
    int kept = 0, same = 0;
    for (int i = lane; i < nl; i += 64) {
        const unsigned long long key = key_load(&keys[i]);
        const int gc = p.lcls[ls + i];
        int row = p.nc;
        if (key) {
            row = (int)dets[min((int)(unsigned)key, cnt - 1)].cls;              // (the low word is a detection below cnt whose class pass 1 found in range)
            ++kept;
            same += row == gc;
        }
        atomicAdd(&p.matrix[row * n1 + gc], 1ULL);
    }
    kept = wave_sum_i32(kept);
    same = wave_sum_i32(same);
    // pass 3: with a kept pair in the image, every detection that takes part and that no label keeps is a background entry
    if (kept > 0)
        for (int d = lane; d < cnt; d += 64) {
            const int l = best[d];                                              // (this lane's own store of pass 1)
            if (l == kNotTakingPart) continue;
            if (l >= 0 && (unsigned)key_load(&keys[l - ls]) == (unsigned)d) continue;
            atomicAdd(&p.matrix[(int)dets[d].cls * n1 + p.nc], 1ULL);
        }
    if (lane == 0) {
        p.image[b * 4 + 0] = nl; p.image[b * 4 + 1] = part; p.image[b * 4 + 2] = kept; p.image[b * 4 + 3] = same;
    }
}

// ---------------------------------------------------------------- scores ----------------------------------------------------------------
constexpr int kScoreThreads = 256, kScorePer = 8, kScoreChunk = kScoreThreads * kScorePer;
constexpr int kScoreMaxX = 128;

struct ScoreParams {
    const unsigned short* bits;    // [n], sorted by (class, -confidence, index)
    const float* conf;             // [n]
    const long long* run_range;    // [C][2]: the run of every class that has labels
    const int* n_l;                // [C]
    const int* run_chunk0;         // [C + 1]: the first chunk of every run
    const double* x;               // [nx]
    const double* px;              // [npx]
    int* tpc;                      // scratch [10][n]
    double* mpre;                  // scratch [10][n]
    int* chunk_sum;                // scratch [10][nchunks]
    int* chunk_pref;
    double* chunk_max;
    double* chunk_suf;
    double* ap;                    // out [C][10]
    double* p_curve;               // out [C][npx]
    double* r_curve;
    double* pr_curve;
    long long n;
    int C, nchunks, nx, npx;
};

struct ScoreChunk { long long run_begin, begin, end; };   // elements [begin, end) of the sorted arrays, inside the run that starts at run_begin

__device__ __forceinline__ ScoreChunk score_chunk(const ScoreParams& p, int k) {
    int lo = 0, hi = p.C;                                                       // the run with run_chunk0[c] <= k < run_chunk0[c + 1]
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (p.run_chunk0[mid + 1] <= k) lo = mid + 1; else hi = mid;
    }
    ScoreChunk c = {0, 0, 0};
    if (lo >= p.C) return c;
    const long long a = min(max(p.run_range[2 * lo], 0LL), p.n), e = min(max(p.run_range[2 * lo + 1], a), p.n);
    c.run_begin = a;
    c.begin = min(a + (long long)(k - p.run_chunk0[lo]) * kScoreChunk, e);
    c.end = min(c.begin + kScoreChunk, e);
    return c;
}

// exclusive prefix of v over the workgroup's 256 threads in thread order; *total = the sum (lds: 4 ints)
__device__ __forceinline__ int block_scan_i32(int v, int* lds, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const int t = __shfl_up(incl, s, 64);
        if (lane >= s) incl += t;
    }
    __syncthreads();
    if (lane == 63) lds[wave] = incl;
    __syncthreads();
    int off = 0, all = 0;
    for (int w = 0; w < kScoreThreads / 64; ++w) {
        if (w < wave) off += lds[w];
        all += lds[w];
    }
    *total = all;
    return off + incl - v;
}

// the maximum of v over the threads after this one (0 without any: precision is never negative); *total = the maximum over all (lds: 4 doubles)
__device__ __forceinline__ double block_suffix_max_f64(double v, double* lds, double* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double incl = v;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const double t = __shfl_down(incl, s, 64);
        if (lane + s < 64) incl = t > incl ? t : incl;
    }
    double after = __shfl_down(incl, 1, 64);                                    // the lanes after this one
    if (lane == 63) after = 0.0;
    __syncthreads();
    if (lane == 0) lds[wave] = incl;
    __syncthreads();
    double all = 0.0;
    for (int w = 0; w < kScoreThreads / 64; ++w) {
        const double t = lds[w];
        if (w > wave) after = t > after ? t : after;
        all = t > all ? t : all;
    }
    *total = all;
    return after;
}

__global__ __launch_bounds__(kScoreThreads) void score_sums_kernel(const ScoreParams p) {
    __shared__ int lds[4];
    const int j = blockIdx.y;
    const ScoreChunk c = score_chunk(p, blockIdx.x);
    int s = 0;
    const long long first = c.begin + (long long)threadIdx.x * kScorePer;
    for (int e = 0; e < kScorePer; ++e)
        if (first + e < c.end) s += (p.bits[first + e] >> j) & 1;
    int total;
    block_scan_i32(s, lds, &total);
    if (threadIdx.x == 0) p.chunk_sum[(long long)j * p.nchunks + blockIdx.x] = total;
}

// per (run, threshold), one wavefront: the carried prefix (SUFFIX = false: exclusive sums of chunk_sum from the left) or the carried suffix
// (SUFFIX = true: exclusive maxima of chunk_max from the right, 0 after the last chunk)
template <bool SUFFIX>
__global__ __launch_bounds__(64) void score_carry_kernel(const ScoreParams p) {
    const int c = blockIdx.x, j = blockIdx.y, lane = threadIdx.x;
    const int k0 = min(max(p.run_chunk0[c], 0), p.nchunks), k1 = min(max(p.run_chunk0[c + 1], k0), p.nchunks);
    const long long row = (long long)j * p.nchunks;
    if (!SUFFIX) {
        int carry = 0;
        for (int base = k0; base < k1; base += 64) {                            // uniform trip count
            const int k = base + lane;
            const int v = k < k1 ? p.chunk_sum[row + k] : 0;
            int incl = v;
#pragma unroll
            for (int s = 1; s < 64; s <<= 1) {
                const int t = __shfl_up(incl, s, 64);
                if (lane >= s) incl += t;
            }
            if (k < k1) p.chunk_pref[row + k] = carry + incl - v;
            carry += __shfl(incl, 63, 64);
        }
    } else {
        double carry = 0.0;
        for (int top = k1; top > k0; top -= 64) {                               // lane l takes chunk top - 1 - l: from the right
            const int k = top - 1 - lane;
            const double v = k >= k0 ? p.chunk_max[row + k] : 0.0;
            double incl = v;
#pragma unroll
            for (int s = 1; s < 64; s <<= 1) {
                const double t = __shfl_up(incl, s, 64);
                if (lane >= s) incl = t > incl ? t : incl;
            }
            double before = __shfl_up(incl, 1, 64);                             // the chunks to the right of this one within the 64
            if (lane == 0) before = 0.0;
            before = carry > before ? carry : before;
            if (k >= k0) p.chunk_suf[row + k] = before;
            const double all = __shfl(incl, 63, 64);
            carry = all > carry ? all : carry;
        }
    }
}

__global__ __launch_bounds__(kScoreThreads) void score_tpc_kernel(const ScoreParams p) {
    __shared__ int lds[4];
    __shared__ double ldsd[4];
    const int j = blockIdx.y;
    const ScoreChunk c = score_chunk(p, blockIdx.x);
    const long long first = c.begin + (long long)threadIdx.x * kScorePer;
    int bit[kScorePer], s = 0;
    for (int e = 0; e < kScorePer; ++e) {
        bit[e] = first + e < c.end ? (p.bits[first + e] >> j) & 1 : 0;
        s += bit[e];
    }
    int total;
    int run = block_scan_i32(s, lds, &total) + p.chunk_pref[(long long)j * p.nchunks + blockIdx.x];
    double mx = 0.0;
    for (int e = 0; e < kScorePer; ++e) {
        if (first + e < c.end) {
            run += bit[e];
            p.tpc[(long long)j * p.n + first + e] = run;
            const double prec = (double)run / (double)(first + e - c.run_begin + 1);
            mx = prec > mx ? prec : mx;
        }
    }
    double all;
    block_suffix_max_f64(mx, ldsd, &all);
    if (threadIdx.x == 0) p.chunk_max[(long long)j * p.nchunks + blockIdx.x] = all;
}

__global__ __launch_bounds__(kScoreThreads) void score_mpre_kernel(const ScoreParams p) {
    __shared__ double ldsd[4];
    const int j = blockIdx.y;
    const ScoreChunk c = score_chunk(p, blockIdx.x);
    const long long first = c.begin + (long long)threadIdx.x * kScorePer;
    double suf[kScorePer], mx = 0.0;
    for (int e = kScorePer - 1; e >= 0; --e) {                                  // this thread's own running maximum from the right
        if (first + e < c.end) {
            const double prec = (double)p.tpc[(long long)j * p.n + first + e] / (double)(first + e - c.run_begin + 1);
            mx = prec > mx ? prec : mx;
        }
        suf[e] = mx;
    }
    double all;
    double after = block_suffix_max_f64(mx, ldsd, &all);
    const double carried = p.chunk_suf[(long long)j * p.nchunks + blockIdx.x];
    after = carried > after ? carried : after;
    for (int e = 0; e < kScorePer; ++e)
        if (first + e < c.end) p.mpre[(long long)j * p.n + first + e] = suf[e] > after ? suf[e] : after;
}

// np.interp's rule: j = the last index with xp[j] <= x; fp[j] when j is the last index or xp[j] == x, else the line through the knots j and
// j + 1, in this order of operations.  x below xp[0]: left; above xp[len - 1]: fp[len - 1].  len >= 1.
template <typename XP, typename FP>
__device__ __forceinline__ double interp_rule(double x, long long len, XP xp, FP fp, double left) {
    if (x > xp(len - 1)) return fp(len - 1);
    if (x < xp(0)) return left;
    long long lo = 0, hi = len;                                                 // the first index with xp > x
    while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (xp(mid) <= x) lo = mid + 1; else hi = mid;
    }
    const long long j = lo - 1;
    const double xj = xp(j), fj = fp(j);
    if (j == len - 1 || xj == x) return fj;
    return (fp(j + 1) - fj) / (xp(j + 1) - xj) * (x - xj) + fj;
}

__global__ __launch_bounds__(kScoreThreads) void score_ap_kernel(const ScoreParams p) {
    __shared__ double y[kScoreMaxX];
    const int c = blockIdx.x, j = blockIdx.y, tid = threadIdx.x;
    const long long a = min(max(p.run_range[2 * c], 0LL), p.n), e = min(max(p.run_range[2 * c + 1], a), p.n);
    const long long n = e - a;
    if (n == 0) {                                                               // labels but no detection: upstream leaves zeros (uniform)
        if (tid == 0) p.ap[c * 10 + j] = 0.0;
        if (j == 0)
            for (int i = tid; i < p.npx; i += kScoreThreads) {
                p.p_curve[(long long)c * p.npx + i] = 0.0;
                p.r_curve[(long long)c * p.npx + i] = 0.0;
                p.pr_curve[(long long)c * p.npx + i] = 0.0;
            }
        return;
    }
    const int* tpc = p.tpc + (long long)j * p.n + a;
    const double* mp = p.mpre + (long long)j * p.n + a;
    const float* conf = p.conf + a;
    const double denom = (double)p.n_l[c] + 1e-16;
    auto recall = [&](long long k) { return (double)tpc[k] / denom; };
    auto precision = [&](long long k) { return (double)tpc[k] / (double)(k + 1); };
    auto mrec = [&](long long i) { return i == 0 ? 0.0 : (i == n + 1 ? 1.0 : recall(i - 1)); };
    auto mpre = [&](long long i) { return i == 0 ? (mp[0] > 1.0 ? mp[0] : 1.0) : (i == n + 1 ? 0.0 : mp[i - 1]); };
    auto nconf = [&](long long k) { return -(double)conf[k]; };
    for (int i = tid; i < p.nx; i += kScoreThreads) y[i] = interp_rule(p.x[i], n + 2, mrec, mpre, 1.0);
    __syncthreads();
    if (tid == 0) {                                                             // the trapezoid sum, one term at a time in ascending x
        double s = 0.0;
        for (int i = 0; i + 1 < p.nx; ++i) s += (p.x[i + 1] - p.x[i]) * (y[i + 1] + y[i]) / 2.0;
        p.ap[c * 10 + j] = s;
    }
    if (j == 0)
        for (int i = tid; i < p.npx; i += kScoreThreads) {
            const double v = p.px[i];
            p.r_curve[(long long)c * p.npx + i] = interp_rule(-v, n, nconf, recall, 0.0);
            p.p_curve[(long long)c * p.npx + i] = interp_rule(-v, n, nconf, precision, 1.0);
            p.pr_curve[(long long)c * p.npx + i] = interp_rule(v, n + 2, mrec, mpre, 1.0);
        }
}

size_t align8(size_t v) { return (v + 7) & ~(size_t)7; }

}  // namespace

extern "C" size_t aq_val_expand_scratch_bytes(int B, int N, int nc) {
    if (B < 1 || N < 1 || nc < 1 || !sg::val_count_fits((long long)N * nc)) return 0;
    const long long nchunks = ((long long)N * nc + kExpandChunk - 1) / kExpandChunk;
    return (size_t)(B * nchunks + 1) * sizeof(int);
}

extern "C" int aq_val_expand_rows_f32(const float* pred_dev, int B, int N, int nc, float conf_thres, int M, void* scratch_dev,
                                      size_t scratch_bytes, float* rows_dev, int32_t* count_dev, void* stream) {
    AQ_REQUIRE(B >= 1 && B <= 65535 && N >= 1 && nc >= 1 && sg::val_count_fits((long long)N * nc),
               "val expand: %d images (1 to 65535), %d rows x %d classes (at least one of each, the product below 2^31)", B, N, nc);
    AQ_REQUIRE(M >= 1 && M <= (long long)N * nc, "val expand: M = %d output rows per image (1 to N x nc = %lld)", M, (long long)N * nc);
    AQ_REQUIRE(conf_thres >= 0.f && conf_thres <= 1.f, "val expand: conf_thres %g (0 to 1)", conf_thres);
    AQ_REQUIRE(pred_dev && rows_dev && count_dev && scratch_dev, "val expand: null pointer");
    AQ_REQUIRE(((uintptr_t)pred_dev & 3) == 0 && ((uintptr_t)rows_dev & 3) == 0 && ((uintptr_t)count_dev & 3) == 0 && ((uintptr_t)scratch_dev & 3) == 0,
               "val expand: unaligned array");
    AQ_REQUIRE(scratch_bytes >= aq_val_expand_scratch_bytes(B, N, nc), "val expand: scratch of %zu bytes, %zu needed", scratch_bytes,
               aq_val_expand_scratch_bytes(B, N, nc));
    ExpandParams p = {};
    p.pred = pred_dev; p.rows = rows_dev; p.counts = count_dev;
    p.B = B; p.N = N; p.nc = nc; p.no = 5 + nc; p.M = M; p.pairs = (long long)N * nc;
    p.nchunks = (int)((p.pairs + kExpandChunk - 1) / kExpandChunk);
    p.chunk_count = (int*)scratch_dev;
    p.overflow = p.chunk_count + (size_t)B * p.nchunks;
    p.conf = conf_thres;
    const dim3 grid((unsigned)p.nchunks, (unsigned)B);
    hipLaunchKernelGGL(expand_count_kernel, grid, dim3(kExpandChunk), 0, (hipStream_t)stream, p);
    hipLaunchKernelGGL(expand_totals_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, (hipStream_t)stream, p);
    hipLaunchKernelGGL(expand_write_kernel, grid, dim3(kExpandChunk), 0, (hipStream_t)stream, p);
    AQ_CHECK_HIP(hipGetLastError());
    return AQ_OK;
}

extern "C" int aq_val_match(const aq_det* dets_dev, const int32_t* counts_dev, int B, int max_det, const float* label_box_dev,
                            const int32_t* label_cls_dev, const int32_t* label_start_dev, const int32_t* label_start_host, long long L,
                            const float* geom_dev, const float* iouv_host, int32_t* scratch_dev, float* conf_out_dev, int32_t* cls_out_dev,
                            uint16_t* bits_out_dev, long long cap, long long* total_dev, void* stream) {
    AQ_REQUIRE(B >= 0 && B <= 65535 && max_det >= 1 && sg::val_count_fits((long long)B * max_det) && sg::val_count_fits(L * 10) && cap >= 0,
               "val match: %d images (0 to 65535), max_det %d, %lld labels (10 x labels below 2^31), capacity %lld", B, max_det, L, cap);
    if (B == 0) return AQ_OK;
    AQ_REQUIRE(label_start_host && iouv_host, "val match: null pointer (the host copies of the label starts and the thresholds)");
    for (int b = 0; b <= B; ++b)
        AQ_REQUIRE(label_start_host[b] >= 0 && label_start_host[b] <= L && (b == 0 || label_start_host[b] >= label_start_host[b - 1]),
                   "val match: label start %d is %d (sorted, inside [0, %lld])", b, label_start_host[b], L);
    AQ_REQUIRE(dets_dev && counts_dev && label_start_dev && geom_dev && total_dev && (L == 0 || (label_box_dev && label_cls_dev && scratch_dev)) &&
               (cap == 0 || (conf_out_dev && cls_out_dev && bits_out_dev)), "val match: null pointer");
    AQ_REQUIRE(((uintptr_t)dets_dev & 3) == 0 && ((uintptr_t)counts_dev & 3) == 0 && ((uintptr_t)label_box_dev & 15) == 0 &&
               ((uintptr_t)label_cls_dev & 3) == 0 && ((uintptr_t)label_start_dev & 3) == 0 && ((uintptr_t)geom_dev & 3) == 0 &&
               ((uintptr_t)scratch_dev & 3) == 0 && ((uintptr_t)conf_out_dev & 3) == 0 && ((uintptr_t)cls_out_dev & 3) == 0 &&
               ((uintptr_t)bits_out_dev & 1) == 0 && ((uintptr_t)total_dev & 7) == 0, "val match: unaligned array");
    MatchParams p = {};
    p.dets = dets_dev; p.counts = counts_dev; p.lbox = (const float4*)label_box_dev; p.lcls = label_cls_dev; p.lstart = label_start_dev;
    p.geom = geom_dev; p.scratch = scratch_dev; p.conf_out = conf_out_dev; p.cls_out = cls_out_dev; p.bits_out = bits_out_dev;
    p.total = total_dev; p.cap = cap; p.B = B; p.max_det = max_det; p.L = (int)L;
    for (int i = 0; i < 10; ++i) p.iouv[i] = iouv_host[i];
    hipLaunchKernelGGL(match_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, p);
    hipLaunchKernelGGL(match_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, p);
    AQ_CHECK_HIP(hipGetLastError());
    return AQ_OK;
}

extern "C" size_t aq_val_confusion_scratch_bytes(int B, int max_det, long long L) {
    if (B < 0 || max_det < 1 || !sg::val_count_fits((long long)B * max_det) || !sg::val_count_fits(L)) return 0;
    return (size_t)L * sizeof(unsigned long long) + align8((size_t)B * max_det * sizeof(int));
}

extern "C" int aq_val_confusion(const aq_det* dets_dev, const int32_t* counts_dev, int B, int max_det, const float* label_box_dev,
                                const int32_t* label_cls_dev, const int32_t* label_cls_host, const int32_t* label_start_dev,
                                const int32_t* label_start_host, long long L, const float* geom_dev, int nc, float conf, float iou,
                                void* scratch_dev, size_t scratch_bytes, long long* matrix_dev, int32_t* image_dev, int32_t* flag_dev,
                                void* stream) {
    AQ_REQUIRE(B >= 0 && B <= 65535 && max_det >= 1 && sg::val_count_fits((long long)B * max_det) && sg::val_count_fits(L),
               "val confusion: %d images (0 to 65535), max_det %d, %lld labels (below 2^31)", B, max_det, L);
    AQ_REQUIRE(nc >= 1 && nc <= 65535, "val confusion: %d classes (1 to 65535)", nc);
    AQ_REQUIRE(std::isfinite(conf) && std::isfinite(iou) && iou > 0.0f,
               "val confusion: confidence threshold %g (finite), IoU threshold %g (finite, above 0)", conf, iou);
    if (B == 0) return AQ_OK;
    AQ_REQUIRE(label_start_host, "val confusion: null pointer (the host copy of the label starts)");
    for (int b = 0; b <= B; ++b)
        AQ_REQUIRE(label_start_host[b] >= 0 && label_start_host[b] <= L && (b == 0 || label_start_host[b] >= label_start_host[b - 1]),
                   "val confusion: label start %d is %d (sorted, inside [0, %lld])", b, label_start_host[b], L);
    if (label_cls_host)
        for (long long l = 0; l < L; ++l)
            AQ_REQUIRE(label_cls_host[l] >= 0 && label_cls_host[l] < nc, "val confusion: label %lld has class %d (0 to %d)", l, label_cls_host[l], nc - 1);
    AQ_REQUIRE(dets_dev && counts_dev && label_start_dev && geom_dev && matrix_dev && image_dev && flag_dev && scratch_dev &&
               (L == 0 || (label_box_dev && label_cls_dev)), "val confusion: null pointer");
    AQ_REQUIRE(((uintptr_t)dets_dev & 3) == 0 && ((uintptr_t)counts_dev & 3) == 0 && ((uintptr_t)label_box_dev & 15) == 0 &&
               ((uintptr_t)label_cls_dev & 3) == 0 && ((uintptr_t)label_start_dev & 3) == 0 && ((uintptr_t)geom_dev & 3) == 0 &&
               ((uintptr_t)scratch_dev & 7) == 0 && ((uintptr_t)matrix_dev & 7) == 0 && ((uintptr_t)image_dev & 3) == 0 &&
               ((uintptr_t)flag_dev & 3) == 0, "val confusion: unaligned array");
    AQ_REQUIRE(scratch_bytes >= aq_val_confusion_scratch_bytes(B, max_det, L), "val confusion: scratch of %zu bytes, %zu needed", scratch_bytes,
               aq_val_confusion_scratch_bytes(B, max_det, L));
    ConfusionParams p = {};
    p.dets = dets_dev; p.counts = counts_dev; p.lbox = (const float4*)label_box_dev; p.lcls = label_cls_dev; p.lstart = label_start_dev;
    p.geom = geom_dev;
    p.keys = (unsigned long long*)scratch_dev;
    p.best = (int*)((char*)scratch_dev + (size_t)L * sizeof(unsigned long long));
    p.matrix = (unsigned long long*)matrix_dev; p.image = image_dev; p.flag = flag_dev;
    p.B = B; p.max_det = max_det; p.L = (int)L; p.nc = nc; p.conf = conf; p.iou = iou;
    hipLaunchKernelGGL(confusion_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, p);
    AQ_CHECK_HIP(hipGetLastError());
    return AQ_OK;
}

extern "C" int aq_val_score_chunk(void) { return kScoreChunk; }

extern "C" size_t aq_val_scores_scratch_bytes(long long n, long long nchunks) {
    if (!sg::val_count_fits(n) || !sg::val_count_fits(nchunks)) return 0;
    return align8((size_t)n * 10 * sizeof(int)) + (size_t)n * 10 * sizeof(double) + 2 * align8((size_t)nchunks * 10 * sizeof(int)) +
           2 * (size_t)nchunks * 10 * sizeof(double) + 8;
}

extern "C" int aq_val_scores_f64(const uint16_t* bits_dev, const float* conf_dev, long long n, const long long* run_range_dev,
                                 const long long* run_range_host, const int32_t* n_l_dev, const int32_t* run_chunk0_dev,
                                 const int32_t* run_chunk0_host, int C, const double* x_dev, int nx, const double* px_dev, int npx,
                                 void* scratch_dev, size_t scratch_bytes, double* ap_dev, double* p_dev, double* r_dev, double* pr_dev,
                                 void* stream) {
    AQ_REQUIRE(sg::val_count_fits(n) && C >= 0 && C <= 65535 && nx >= 2 && nx <= kScoreMaxX && npx >= 1 && npx <= (1 << 20),
               "val scores: %lld detections (below 2^31), %d classes (0 to 65535), %d integration points (2 to %d), %d curve points (1 to 2^20)",
               n, C, nx, kScoreMaxX, npx);
    if (C == 0) return AQ_OK;
    AQ_REQUIRE(run_range_host && run_chunk0_host, "val scores: null pointer (the host copies of the runs and their first chunks)");
    AQ_REQUIRE(run_chunk0_host[0] == 0, "val scores: the first run's first chunk is %d, not 0", run_chunk0_host[0]);
    for (int c = 0; c < C; ++c) {
        const long long a = run_range_host[2 * c], e = run_range_host[2 * c + 1];
        AQ_REQUIRE(a >= 0 && a <= e && e <= n && (c == 0 || a >= run_range_host[2 * c - 1]), "val scores: run %d is [%lld, %lld) (ascending, inside [0, %lld])", c, a, e, n);
        AQ_REQUIRE(run_chunk0_host[c + 1] - run_chunk0_host[c] == (e - a + kScoreChunk - 1) / kScoreChunk,
                   "val scores: run %d of %lld detections has chunks %d to %d (%d detections per chunk)", c, e - a, run_chunk0_host[c], run_chunk0_host[c + 1], kScoreChunk);
    }
    const int nchunks = run_chunk0_host[C];
    AQ_REQUIRE(run_range_dev && n_l_dev && run_chunk0_dev && x_dev && px_dev && ap_dev && p_dev && r_dev && pr_dev && (n == 0 || (bits_dev && conf_dev)) &&
               scratch_dev, "val scores: null pointer");
    AQ_REQUIRE(((uintptr_t)bits_dev & 1) == 0 && ((uintptr_t)conf_dev & 3) == 0 && ((uintptr_t)run_range_dev & 7) == 0 && ((uintptr_t)n_l_dev & 3) == 0 &&
               ((uintptr_t)run_chunk0_dev & 3) == 0 && ((uintptr_t)x_dev & 7) == 0 && ((uintptr_t)px_dev & 7) == 0 && ((uintptr_t)scratch_dev & 7) == 0 &&
               ((uintptr_t)ap_dev & 7) == 0 && ((uintptr_t)p_dev & 7) == 0 && ((uintptr_t)r_dev & 7) == 0 && ((uintptr_t)pr_dev & 7) == 0,
               "val scores: unaligned array");
    AQ_REQUIRE(scratch_bytes >= aq_val_scores_scratch_bytes(n, nchunks), "val scores: scratch of %zu bytes, %zu needed", scratch_bytes,
               aq_val_scores_scratch_bytes(n, nchunks));
    ScoreParams p = {};
    p.bits = bits_dev; p.conf = conf_dev; p.run_range = run_range_dev; p.n_l = n_l_dev; p.run_chunk0 = run_chunk0_dev; p.x = x_dev; p.px = px_dev;
    char* s = (char*)scratch_dev;
    p.mpre = (double*)s;       s += (size_t)n * 10 * sizeof(double);
    p.chunk_max = (double*)s;  s += (size_t)nchunks * 10 * sizeof(double);
    p.chunk_suf = (double*)s;  s += (size_t)nchunks * 10 * sizeof(double);
    p.tpc = (int*)s;           s += align8((size_t)n * 10 * sizeof(int));
    p.chunk_sum = (int*)s;     s += align8((size_t)nchunks * 10 * sizeof(int));
    p.chunk_pref = (int*)s;
    p.ap = ap_dev; p.p_curve = p_dev; p.r_curve = r_dev; p.pr_curve = pr_dev;
    p.n = n; p.C = C; p.nchunks = nchunks; p.nx = nx; p.npx = npx;
    hipStream_t st = (hipStream_t)stream;
    if (nchunks > 0) {
        const dim3 grid((unsigned)nchunks, 10);
        hipLaunchKernelGGL(score_sums_kernel, grid, dim3(kScoreThreads), 0, st, p);
        hipLaunchKernelGGL(score_carry_kernel<false>, dim3((unsigned)C, 10), dim3(64), 0, st, p);
        hipLaunchKernelGGL(score_tpc_kernel, grid, dim3(kScoreThreads), 0, st, p);
        hipLaunchKernelGGL(score_carry_kernel<true>, dim3((unsigned)C, 10), dim3(64), 0, st, p);
        hipLaunchKernelGGL(score_mpre_kernel, grid, dim3(kScoreThreads), 0, st, p);
    }
    hipLaunchKernelGGL(score_ap_kernel, dim3((unsigned)C, 10), dim3(kScoreThreads), 0, st, p);
    AQ_CHECK_HIP(hipGetLastError());
    return AQ_OK;
}
