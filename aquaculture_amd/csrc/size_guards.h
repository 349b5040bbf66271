// The size guards of the launchers: for each kernel family, the largest batch / image / row length its index arithmetic takes.
// Every limit is written here once.  The launcher's AQ_REQUIRE, the exported *_supported / *_form queries and the engine's batch check
// (plan_unfit_op in engine.cpp) all call these, so the sizing call refuses exactly what a launcher would refuse in the middle of a
// sweep.  oracle/guards.py restates each function in one Python line; tests/test_size_guards.py compares the two at every edge.
//
// Plain host arithmetic on long long: nothing from HIP, no environment switch, no global.  Null-pointer, alignment and slice checks,
// and which channel counts a kernel is built for, stay in the launchers.  B: images; H, W: pixels of the tensor named in the comment;
// *_ld: row length in elements (channels per pixel) unless the comment says bytes.  Every predicate only gets harder to meet as B grows.
#pragma once

namespace sg {

typedef long long ll;

constexpr ll cdiv(ll a, ll b) { return (a + b - 1) / b; }

// Output tiles of the kernels whose guard counts tiles.  Each .hip file asserts its own tile constants against these.
constexpr ll kStemTW = 64, kStemTH = 8;                      // stem_conv.hip
constexpr ll kDownTW = 16, kDownblockTH = 8, kConv3x3s2TH = 4;   // downblock.hip: <48, 96, fused 1x1> and <96, 192>
constexpr ll btl_tile_w(ll C) { return C == 16 ? 32 : 16; }  // bottleneck.hip: the HIP-source shapes and the assembly builds alike
constexpr ll btl_tile_h(ll C) { return C == 96 ? 8 : 16; }

// ---- pointwise.hip ----
// aq_preprocess_s2d on B x H x W tiles: one 32-bit index per output pixel.
inline bool preprocess_fits(ll B, ll H, ll W) { return B * (H / 2) * (W / 2) < (1LL << 31); }
// aq_sppf_pool on B x H x W pixels of `groups` 16-byte channel groups.
inline bool sppf_pool_fits(ll B, ll H, ll W, ll groups) { return B * H * W * groups < (1LL << 31); }
// aq_upsample2x from B x H x W pixels: 32-bit index per output group; one grid row per input row.
inline bool upsample2x_fits(ll B, ll H, ll W, ll groups) { return B * 4 * H * W * groups < (1LL << 31); }
inline bool upsample2x_rows_fit(ll B, ll H) { return B * H < 65536; }

// uint8 RGB source tiles read through 64-bit addresses by the launchers that sample them (aq_stem_conv_scaled, aq_stemdown).
inline bool tile_bytes_fit(ll B, ll H, ll W) { return B * H * W * 3 < (1LL << 40); }

// ---- stem_conv.hip ----
// Output side of both stem launchers (Ho x Wo output pixels): 31-bit pixel and tile indices.
inline bool stem_out_fits(ll B, ll Ho, ll Wo) {
    return B * Ho * Wo < (1LL << 31) && B * cdiv(Wo, kStemTW) * cdiv(Ho, kStemTH) < (1LL << 31);
}
// aq_stem_conv on B x H x W uint8 RGB tiles: 32-bit input byte offsets.
inline bool stem_fits(ll B, ll H, ll W) { return B * H * W * 3 < (1LL << 32) && stem_out_fits(B, H / 2, W / 2); }

// ---- downblock.hip ----  (H x W: the input; tiles of th x 16 output pixels)
inline bool down_fits(ll B, ll H, ll W, ll th) {
    return B * H * W < (1LL << 31) && B * cdiv(W / 2, kDownTW) * cdiv(H / 2, th) < (1LL << 30);
}
inline bool downblock_fits(ll B, ll H, ll W) { return down_fits(B, H, W, kDownblockTH); }            // aq_downblock, aq_stemdown
inline bool conv3x3s2_direct_fits(ll B, ll H, ll W) { return down_fits(B, H, W, kConv3x3s2TH); }     // aq_conv3x3s2_direct

// ---- bottleneck.hip ----
// aq_bottleneck, any build: 31-bit pixel index, 30-bit tile index.
inline bool bottleneck_fits(ll C, ll B, ll H, ll W) {
    return B * H * W < (1LL << 31) && B * cdiv(W, btl_tile_w(C)) * cdiv(H, btl_tile_h(C)) < (1LL << 30);
}
// The generated-assembly builds (C = 48: 16 x 16 tiles, C = 96: 8 x 16): the magic-number tile decode needs two tiles per row and image
// and tile counts under 2^24 / 2^32; 32-bit buffer offsets keep the input slice under 2^30 bytes and the output under 2^31.
inline bool btl_asm_tiles_fit(ll C, ll B, ll H, ll W, ll in_ld, ll out_ld) {
    const ll tx = cdiv(W, 16), tpi = tx * cdiv(H, btl_tile_h(C)), nt = tpi * B;
    return tx >= 2 && tpi >= 2 && nt < (1LL << 24) && nt * tpi < (1LL << 32) &&
           B * H * W * in_ld * 2 < (1LL << 30) && B * H * W * out_ld * 2 < (1LL << 31);
}
// aq_bottleneck_c3tail, on top of btl_asm_tiles_fit(48, ...): 32-bit row offsets into the concat tensor.
inline bool c3tail_cat_fits(ll B, ll H, ll W, ll cat_ld) { return B * H * W * cat_ld * 2 < (1LL << 31); }

// ---- conv1x1_direct.hip, conv1x1_asm.hip ----
inline bool conv1x1_direct_fits(ll npix) { return npix < (1LL << 31); }
// 32-bit buffer offsets; the "no tile left" fetch lands up to 2^22 bytes past the tensor and must not wrap.
inline bool conv1x1_asm_fits(ll npix, ll in_ld, ll out_ld) {
    return npix * in_ld * 2 < (1LL << 31) - (1LL << 22) && npix * out_ld * 2 < (1LL << 32) - (1LL << 22);
}

// ---- conv3x3_pl.hip ----
// The planar kernels' fast pixel index over the padded B x (H + 1) x (W + 1) grid (exact in fp32 up to 2^23).  H x W is the OUTPUT size:
// the stride-2 form passes H / 2, W / 2.
// It also bounds the launchers' tile counts (ntiles < 2^30): at most 2^23 / 16 pixel blocks times cout / 192 <= 5 channel tiles.
inline bool pl3x3_index_fits(ll B, ll H, ll W) { return B * (H + 1) * (W + 1) + W + 2 < (1LL << 23); }
// Stride 1, bf16 / w8: 31-bit byte offsets into the output and residual tensors (res_ld = 0: none).
inline bool pl3x3_offsets_fit(ll B, ll H, ll W, ll out_ld, ll res_ld) {
    return B * H * W * out_ld * 2 < (1LL << 31) && B * H * W * res_ld * 2 < (1LL << 31);
}
// Stride 2 on a B x H x W input: index range of the output grid, 31-bit byte offsets (the input goes through a buffer descriptor of 2^31
// records), 24-bit pixel stride.
inline bool pl3x3s2_fits(ll B, ll H, ll W, ll in_ld, ll out_ld) {
    return pl3x3_index_fits(B, H / 2, W / 2) && B * (H / 2) * (W / 2) * out_ld * 2 < (1LL << 31) && B * H * W * in_ld * 2 < (1LL << 31) &&
           in_ld * 2 < (1LL << 24);
}
// fp8 x fp8: pl3x3_offsets_fit, and the e4m3 input (in_ld_bytes per pixel) under 2^31 bytes with a 24-bit pixel stride.
inline bool pl3x3_f8_offsets_fit(ll B, ll H, ll W, ll in_ld_bytes, ll out_ld, ll res_ld) {
    return pl3x3_offsets_fit(B, H, W, out_ld, res_ld) && B * H * W * in_ld_bytes < (1LL << 31) && in_ld_bytes < (1LL << 24);
}

// ---- conv_igemm.hip, conv_halo.hip ----  (npix = B x Ho x Wo; G 16-byte groups per tap; bm x bn: the tile shape of the config)
inline bool igemm_index_fits(ll npix, ll kgroups_pad, ll G) {
    return npix < (1LL << 24) && kgroups_pad < (1LL << 15) && G > 0 && G < (1LL << 15);
}
inline bool igemm_tiles_fit(ll npix, ll cout, ll bm, ll bn) {   // (tm * tn, the grid's tile count, is below 2^31 with it)
    const ll tm = cdiv(cout, bm), tn = cdiv(npix, bn);
    return tm * tn * tm < (1LL << 31);
}
inline bool igemm_fits(ll npix, ll kgroups_pad, ll G, ll cout, ll bm, ll bn) {
    return igemm_index_fits(npix, kgroups_pad, G) && igemm_tiles_fit(npix, cout, bm, bn);
}

// ---- head_decode.hip ----  (ny x nx: the level's grid)
inline bool head_decode_fits(ll B, ll ny, ll nx) { return B * ny * nx < (1LL << 30); }

// ---- dedup.hip ----  (every count of a call -- ring vertices, rings, bitmap words, groups, cages -- is a 31-bit index; these three have no
// line in oracle/guards.py: tests/test_gpu_dedup.py walks their edges through the launchers' refusals)
constexpr ll kDedupMaxSlots = 5, kDedupMaxPerms = 120;      // images of one (pass, tile key) group: the longest image pass; 5! orders
constexpr ll kDedupMaxSide = 1LL << 15;                     // frame width and height
inline bool dedup_count_fits(ll n) { return n >= 0 && n < (1LL << 31); }
inline bool dedup_frame_fits(ll w, ll h) { return w >= 1 && h >= 1 && w <= kDedupMaxSide && h <= kDedupMaxSide; }
constexpr ll dedup_pitch(ll w) { return cdiv(w + 1, 32); }  // words of a bitmap row: w pixels and the column x = w of the toggles

// ---- coverage.hip ----  (images, ring vertices, band entries, queries and passes of a call are 31-bit indices -- ring_start holds the vertex
// offsets as int32 -- and band_start has P nbands + 1 entries; like dedup's, no line in oracle/guards.py: tests/test_gpu_missing.py walks the
// edges through the launcher's refusals)
inline bool coverage_count_fits(ll n) { return n >= 0 && n < (1LL << 31); }
inline bool coverage_bands_fit(ll P, ll nbands) { return P >= 0 && nbands >= 1 && nbands < (1LL << 31) && P * nbands + 1 < (1LL << 31); }

// ---- model_errors.hip ----  (queries, keys and moment groups of a call are 31-bit indices; like dedup's, no line in oracle/guards.py:
// tests/test_gpu_model_errors.py walks the edge through the launchers' refusals)
inline bool model_error_count_fits(ll n) { return n >= 0 && n < (1LL << 31); }

// ---- eval_subsets.hip ----  (n points, queries or keys of a call: a 31-bit index; the [S][n][K] arrays of doubles are indexed in 64 bits,
// (s n + i) K, and S n K below 2^36 keeps every byte offset and the scratch size below 2^40; K = 0 (a join without payload) counts as 1.  S and
// K are bounded here too (32 bits of a mask word; 16 list slots), so the product below is under 2^40 whatever a caller passes.  Both
// launchers and both scratch queries call it; like dedup's, no line in oracle/guards.py: tests/test_gpu_kfold.py walks the launchers' refusals)
inline bool eval_subsets_fit(ll n, ll K, ll S) {
    return n >= 0 && n < (1LL << 31) && K >= 0 && K <= 16 && S >= 1 && S <= 32 && S * n * (K > 0 ? K : 1) < (1LL << 36);
}

// ---- overlaps.hip ----  (boxes, band entries, list entries and detections of a call are 31-bit indices; band_start has nbands + 1 entries;
// like dedup's, no line in oracle/guards.py: tests/test_gpu_overlaps.py walks the edges through the launchers' refusals)
inline bool overlap_count_fits(ll n) { return n >= 0 && n < (1LL << 31); }
inline bool overlap_bands_fit(ll nbands) { return nbands >= 1 && nbands + 1 < (1LL << 31); }

// ---- facility_sites.hip ----  (facilities, entries, queries, keys, groups and list entries of a call are 31-bit indices; like dedup's, no
// line in oracle/guards.py: tests/test_gpu_facility_sites.py walks the edge through the launchers' refusals)
inline bool facility_sites_count_fits(ll n) { return n >= 0 && n < (1LL << 31); }

// ---- val.hip ----  (images, (row, class) pairs, labels and detections of a call are 31-bit indices; the row arrays [B][M][5 + nc] are
// indexed in 64 bits; like dedup's, no line in oracle/guards.py: tests/test_gpu_val.py walks the launchers' refusals)
inline bool val_count_fits(ll n) { return n >= 0 && n < (1LL << 31); }

// ---- mosaic.hip ----  (n images of H x W in an ns x ns grid, each cell h x w after the resize: upstream's plot_images takes 16 images at the
// most; source mosaic coordinates, output pixels and output bytes are 31-bit values; like dedup's, no line in oracle/guards.py:
// tests/test_gpu_val_plots.py walks the launcher's refusals)
constexpr ll kMosaicMaxImages = 16;
inline bool mosaic_fits(ll n, ll ns, ll H, ll W, ll h, ll w) {
    return n >= 1 && n <= kMosaicMaxImages && ns >= 1 && ns <= 4 && ns * ns >= n && H >= 1 && W >= 1 && h >= 1 && w >= 1 &&
           H < (1LL << 24) && W < (1LL << 24) && h < (1LL << 24) && w < (1LL << 24) &&
           n * H * W * 3 < (1LL << 31) && ns * h * ns * w * 3 < (1LL << 31);
}

}  // namespace sg
