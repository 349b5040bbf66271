// --blank-key: the statistics behind the reference's white-space key (reference src/utils.py is_blank, is_partly_blank and the mask of
// correct_partly_blank_geom), taken from the decoded uint8 RGB images of a batch while they lie in HBM.  One read of every image, a few
// words written per image, integer arithmetic throughout:
//   L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16 per pixel (Pillow's convert("L")), its minimum and maximum (getextrema());
//   blank_rows = rows whose sum over all 3 w bytes is >= 750 w, blank_cols = columns whose sum over all 3 h bytes is >= 750 h
//   (np.average(im, axis=(1, 2)) >= 250. and axis=(0, 2), in integers);
//   nonblank_px = pixels with max(R, G, B) < 250, and their bounding box.
//
// Three launches on the caller's stream: init (the scratch's accumulators and column sums), the sweep, and a finalising kernel (one workgroup
// per image: column sums against 750 h, one record per image).  The sweep gives a workgroup a band of 32 rows of one image, a wave eight of
// them; a lane reads a row in pieces of 16 pixels (48 bytes, three 16-byte loads), so a 1024-px row is one wave-wide piece.  Row sums are
// reduced across the wave and kept per row in LDS across the pieces; column sums are per-lane registers over the wave's rows, combined across the
// four waves in LDS and added to the scratch with one integer atomic per column and band; extrema, count and box are reduced per wave, per
// workgroup, then with integer atomics.  Only integer atomics: the result does not depend on scheduling.  The last, partial piece of a row
// whose width is not a multiple of 16 is read byte by byte; bases and pitches need no alignment.
#include "aq_common.h"
#include <limits.h>

namespace {

constexpr int kBandRows = 32, kWaveRows = 8, kPiecePx = 16, kPieceCols = 64 * kPiecePx, kSlab = kPiecePx * 65;
constexpr int kAcc = 8;    // per image in the scratch: l_min, l_max, blank_rows, nonblank_px, x0, y0, x1, y1

struct BlankParams {
    const unsigned char* img;
    const aq_frame* frames;
    int n_frames;
    int* acc;               // [n_frames][kAcc]
    unsigned* cols;         // column sums, frame i's from frames[i].mcu
    long long n_cols;
    aq_blank_stat* out;
};

struct Piece { unsigned d[12]; };

__device__ __forceinline__ unsigned byte_of(const Piece& v, int i) { return (v.d[i >> 2] >> (8 * (i & 3))) & 255u; }

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
__device__ __forceinline__ unsigned wave_sum(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// One lane's 16 pixels of one row: column sums, grey extrema, the mask of pixels below 250.  FULL: all 16 are inside the row; else the first n
// (the bytes beyond them are zero: nothing for the sums, L = 0 is neutral for the maximum).
template <bool FULL>
__device__ __forceinline__ void take_piece(const Piece& v, int n, unsigned (&col)[kPiecePx], int& l_min, int& l_max, unsigned& mask) {
#pragma unroll
    for (int j = 0; j < kPiecePx; ++j) {
        const unsigned r = byte_of(v, 3 * j), g = byte_of(v, 3 * j + 1), b = byte_of(v, 3 * j + 2);
        col[j] += r + g + b;
        const int l = (int)((19595u * r + 38470u * g + 7471u * b + 0x8000u) >> 16);
        l_min = min(l_min, FULL || j < n ? l : 255);
        l_max = max(l_max, l);
        mask |= (max(r, max(g, b)) < 250u ? 1u : 0u) << j;
    }
    if (!FULL) mask &= (1u << max(n, 0)) - 1u;
}

__global__ __launch_bounds__(256) void blank_init_kernel(const BlankParams p) {
    const long long n_acc = (long long)p.n_frames * kAcc;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n_acc + p.n_cols; i += gridDim.x * 256LL) {
        if (i >= n_acc) { p.cols[i - n_acc] = 0u; continue; }
        const int f = (int)(i & (kAcc - 1));
        p.acc[i] = f == 0 ? 255 : (f == 4 || f == 5) ? INT_MAX : (f == 6 || f == 7) ? -1 : 0;
    }
}

__global__ __launch_bounds__(256) void blank_sweep_kernel(const BlankParams p) {
    __shared__ unsigned slab[4][kSlab];
    __shared__ int part[4][kAcc];
    __shared__ unsigned row_sum[4][kWaveRows];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int fi = blockIdx.y; fi < p.n_frames; fi += gridDim.y) {
        const aq_frame f = p.frames[fi];
        const int bands = (f.h + kBandRows - 1) / kBandRows, pieces = (f.w + kPieceCols - 1) / kPieceCols;
        for (int band = blockIdx.x; band < bands; band += gridDim.x) {
            const int y_first = band * kBandRows + wave * kWaveRows;
            if (lane < kWaveRows) row_sum[wave][lane] = 0u;              // (the wave's own words: no other wave reads them)
            int l_min = 255, l_max = 0, npx = 0, x0 = INT_MAX, y0 = INT_MAX, x1 = -1, y1 = -1;
            for (int pc = 0; pc < pieces; ++pc) {
                const int xb = pc * kPieceCols + lane * kPiecePx;       // this lane's first pixel of the piece
                const int n = min(kPiecePx, f.w - xb);                  // its pixels inside the row (<= 0: none)
                unsigned col[kPiecePx];
#pragma unroll
                for (int j = 0; j < kPiecePx; ++j) col[j] = 0u;
#pragma unroll 2
                for (int i = 0; i < kWaveRows; ++i) {
                    const int y = y_first + i;
                    if (y >= f.h) break;
                    const unsigned char* s = p.img + f.base + (long long)y * f.pitch + 3LL * xb;
                    Piece v;
                    unsigned mask = 0u;
                    if (n == kPiecePx) {
                        __builtin_memcpy(&v, s, 48);
                        take_piece<true>(v, n, col, l_min, l_max, mask);
                    } else {                                            // the row's last, partial piece: bytes beyond it are not read
#pragma unroll
                        for (int k = 0; k < 12; ++k) v.d[k] = 0u;
                        if (n > 0) {                                    // (a loop that is not unrolled, last byte first: the piece moves up a byte per step)
#pragma unroll 1
                            for (int k = 3 * n - 1; k >= 0; --k) {
#pragma unroll
                                for (int q = 11; q > 0; --q) v.d[q] = (v.d[q] << 8) | (v.d[q - 1] >> 24);
                                v.d[0] = (v.d[0] << 8) | s[k];
                            }
                        }
                        take_piece<false>(v, n, col, l_min, l_max, mask);
                    }
                    unsigned sum = 0u;
#pragma unroll
                    for (int k = 0; k < 12; ++k) sum = __builtin_amdgcn_sad_u8(v.d[k], 0u, sum);
                    sum = wave_sum(sum);
                    if (lane == 0) row_sum[wave][i] += sum;
                    if (mask) {
                        npx += __popc(mask);
                        x0 = min(x0, xb + __ffs(mask) - 1);
                        x1 = max(x1, xb + 31 - __clz(mask));
                        y0 = min(y0, y);
                        y1 = max(y1, y);
                    }
                }
                // column sums of this piece and band: the four waves' registers through LDS, one atomic per column
                __syncthreads();
#pragma unroll
                for (int j = 0; j < kPiecePx; ++j) slab[wave][j * 65 + lane] = col[j];
                __syncthreads();
                for (int c = threadIdx.x; c < kPieceCols; c += 256) {
                    const int x = pc * kPieceCols + c, at = (c & 15) * 65 + (c >> 4);
                    if (x >= f.w) break;
                    const unsigned t = slab[0][at] + slab[1][at] + slab[2][at] + slab[3][at];
                    if (t) atomicAdd(p.cols + f.mcu + x, t);
                }
            }
            // rows: each of the wave's rows is complete now
            const unsigned row_bound = 750u * (unsigned)f.w;
            const int rows = (int)wave_sum(lane < kWaveRows && y_first + lane < f.h && row_sum[wave][lane] >= row_bound ? 1u : 0u);
            l_min = wave_min(l_min); l_max = wave_max(l_max); npx = (int)wave_sum((unsigned)npx);
            x0 = wave_min(x0); y0 = wave_min(y0); x1 = wave_max(x1); y1 = wave_max(y1);
            __syncthreads();
            if (lane == 0) {
                part[wave][0] = l_min; part[wave][1] = l_max; part[wave][2] = rows; part[wave][3] = npx;
                part[wave][4] = x0; part[wave][5] = y0; part[wave][6] = x1; part[wave][7] = y1;
            }
            __syncthreads();
            if (threadIdx.x < kAcc) {
                const int k = threadIdx.x;
                const int a = part[0][k], b = part[1][k], c = part[2][k], d = part[3][k];
                int* dst = p.acc + (long long)fi * kAcc + k;
                if (k == 0 || k == 4 || k == 5) {
                    const int v = min(min(a, b), min(c, d));
                    if (v != (k == 0 ? 255 : INT_MAX)) atomicMin(dst, v);
                } else if (k == 1 || k == 6 || k == 7) {
                    const int v = max(max(a, b), max(c, d));
                    if (v != (k == 1 ? 0 : -1)) atomicMax(dst, v);
                } else {
                    const int v = a + b + c + d;
                    if (v) atomicAdd(dst, v);
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void blank_final_kernel(const BlankParams p) {
    __shared__ int part[4];
    for (int fi = blockIdx.x; fi < p.n_frames; fi += gridDim.x) {
        const aq_frame f = p.frames[fi];
        const unsigned bound = 750u * (unsigned)f.h;
        int n = 0;
        for (int x = threadIdx.x; x < f.w; x += 256) n += p.cols[f.mcu + x] >= bound ? 1 : 0;
        n = (int)wave_sum((unsigned)n);
        __syncthreads();
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = n;
        __syncthreads();
        if (threadIdx.x == 0) {
            const int* a = p.acc + (long long)fi * kAcc;
            aq_blank_stat s;
            s.l_min = a[0]; s.l_max = a[1]; s.blank_rows = a[2]; s.blank_cols = part[0] + part[1] + part[2] + part[3]; s.nonblank_px = a[3];
            const bool any = a[3] > 0;                      // no pixel below 250: the empty box (w, h, -1, -1)
            s.x0 = any ? a[4] : f.w; s.y0 = any ? a[5] : f.h; s.x1 = any ? a[6] : -1; s.y1 = any ? a[7] : -1;
            p.out[fi] = s;
        }
    }
}

// The table's checks, shared by the two entry points: columns (and so scratch words) of the frames, or -1 with the error set.
long long check_frames(const aq_frame* frames_host, int n_frames, long long image_bytes, bool check_window) {
    long long cols = 0;
    for (int i = 0; i < n_frames; ++i) {
        const aq_frame& f = frames_host[i];
        if (!(f.w > 0 && f.h > 0 && f.w <= 65535 && f.h <= 65535 && (long long)f.w * f.h <= INT_MAX && f.base >= 0 && f.pitch >= 3LL * f.w)) {
            aq_set_error("blank_stats: frame %d (%d x %d, pitch %d, at byte %lld) is empty, too large or narrower than its pitch", i, f.w, f.h, f.pitch,
                         (long long)f.base);
            return -1;
        }
        if (check_window && f.base + (long long)(f.h - 1) * f.pitch + 3LL * f.w > image_bytes) {
            aq_set_error("blank_stats: frame %d (%d x %d, pitch %d, at byte %lld) leaves its buffer of %lld bytes", i, f.w, f.h, f.pitch,
                         (long long)f.base, image_bytes);
            return -1;
        }
        if (check_window && f.mcu != cols) {
            aq_set_error("blank_stats: frame %d has its column sums at word %d, not where frame %d's end (%lld)", i, f.mcu, i - 1, cols);
            return -1;
        }
        cols += f.w;
        if (cols > INT_MAX) {
            aq_set_error("blank_stats: more than 2^31 columns in one call");
            return -1;
        }
    }
    return cols;
}

}  // namespace

// Bytes of scratch aq_blank_stats_u8 needs for these frames (eight accumulators per frame and one word per column); 0 for no frames or a table
// the call would refuse.
extern "C" size_t aq_blank_stats_scratch_bytes(const aq_frame* frames_host, int n_frames) {
    if (!frames_host || n_frames <= 0) return 0;
    const long long cols = check_frames(frames_host, n_frames, 0, false);
    return cols < 0 ? 0 : (size_t)((long long)n_frames * kAcc + cols) * 4;
}

// Statistics of n_frames images of one buffer.  frames[i].mcu = the frame's first word among the column sums: the frames' columns follow each
// other from 0.  frames_host = frames_dev's content in host memory: a frame that leaves [images_dev, images_dev + image_bytes) is refused before
// anything is launched.  The call initialises its scratch itself and allocates nothing; everything is recorded on `stream`.
extern "C" int aq_blank_stats_u8(const uint8_t* images_dev, long long image_bytes, const aq_frame* frames_dev, const aq_frame* frames_host,
                                 int n_frames, void* scratch_dev, size_t scratch_bytes, aq_blank_stat* stats_dev, void* stream) {
    AQ_REQUIRE(n_frames >= 0, "blank_stats: bad number of frames (%d)", n_frames);
    if (n_frames == 0) return AQ_OK;
    AQ_REQUIRE(images_dev && frames_dev && frames_host && scratch_dev && stats_dev && image_bytes > 0, "blank_stats: null pointer");
    AQ_REQUIRE(((uintptr_t)frames_dev & 7) == 0 && ((uintptr_t)scratch_dev & 3) == 0 && ((uintptr_t)stats_dev & 3) == 0, "blank_stats: unaligned table");
    const long long cols = check_frames(frames_host, n_frames, image_bytes, true);
    if (cols < 0) return AQ_ERR_INVALID;
    const size_t need = (size_t)((long long)n_frames * kAcc + cols) * 4;
    AQ_REQUIRE(scratch_bytes >= need, "blank_stats: %zu bytes of scratch, %zu needed (aq_blank_stats_scratch_bytes)", scratch_bytes, need);
    int max_bands = 1;
    for (int i = 0; i < n_frames; ++i) max_bands = max(max_bands, (frames_host[i].h + kBandRows - 1) / kBandRows);
    int cus = 0;
    AQ_CHECK_HIP(aq_cus(&cus));
    BlankParams p;
    p.img = images_dev; p.frames = frames_dev; p.n_frames = n_frames; p.acc = (int*)scratch_dev; p.cols = (unsigned*)scratch_dev + (size_t)n_frames * kAcc;
    p.n_cols = cols; p.out = stats_dev;
    const long long words = (long long)n_frames * kAcc + cols, init_blocks = (words + 255) / 256;
    hipLaunchKernelGGL(blank_init_kernel, dim3((unsigned)(init_blocks < 8LL * cus ? init_blocks : 8LL * cus)), dim3(256), 0, (hipStream_t)stream, p);
    AQ_CHECK_HIP(hipGetLastError());
    const unsigned gy = (unsigned)min(n_frames, 1024), gx = (unsigned)min(max_bands, max(1, 32 * cus / (int)gy));
    hipLaunchKernelGGL(blank_sweep_kernel, dim3(gx, gy), dim3(256), 0, (hipStream_t)stream, p);
    AQ_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(blank_final_kernel, dim3((unsigned)min(n_frames, 32 * cus)), dim3(256), 0, (hipStream_t)stream, p);
    AQ_CHECK_HIP(hipGetLastError());
    return AQ_OK;
}
