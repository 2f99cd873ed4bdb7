/*
 * sdnet_hip.h -- C ABI of libsdnet_hip.so: the MI355X (gfx950) implementation of the SDNet
 * hot path of laclouis5/StructureDetector.
 *
 * The reference has no FFI layer: this path sits behind plain Python classes
 * (SURVEY.md 8b).  Each entry point below therefore cites the reference *Python* interface it
 * replaces (paths relative to the reference repository root); INTEGRATION.md shows the ctypes
 * stub a reference maintainer would add at each of those sites.
 *
 * Conventions
 *   - plain pointers and sizes only, no torch / C++ types;
 *   - every pointer is a DEVICE pointer unless the name ends in _host;
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream); every call is
 *     asynchronous with respect to the host and performs no allocation and no synchronisation;
 *   - scratch memory comes from the caller: ask sd_*_workspace_bytes(), pass a device buffer;
 *   - return value: 0 = ok, <0 = invalid argument (SD_ERR_*), >0 = hipError_t;
 *     sd_last_error() returns a thread-local message for the last non-zero return;
 *   - maps are fp32, rows contiguous (x stride 1, y stride w); batch / channel strides are
 *     explicit (in elements) so that channel-slice views of the head output
 *     (src/sdnet/model/network.py:77-84) are consumed without a copy.
 */
#ifndef SDNET_HIP_H
#define SDNET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SD_ERR_INVALID   (-1)   /* bad shape / null pointer / unsupported size */
#define SD_ERR_WORKSPACE (-2)   /* workspace too small */
#define SD_ERR_ALIGN     (-3)   /* pointer or stride not 16-byte aligned where required */

#define SD_MAX_TOPK 1024        /* max_objects / max_parts upper bound supported by the select kernel */

typedef void* sd_stream_t;

int         sd_version(void);
const char* sd_last_error(void);
/* Bit mask of timing-only experiment switches compiled into this library (csrc/sd_conv.hip SD_ABLATE_HOT = 1, _STORE = 2,
 * _PATCH = 4: each makes the conv kernels compute WRONG results on purpose).  0 for every product build; the Python loader
 * (structuredetector_amd/_lib.py) refuses a non-zero library.  No reference counterpart (build hygiene). */
int         sd_build_flags(void);

/* ---- tensor primitives: src/sdnet/utils/utils.py ------------------------------------------ */

/* clamped_sigmoid, utils.py:355-361: y = clamp(sigmoid(x), 1e-6, 1-1e-6); n contiguous floats. */
int sd_clamped_sigmoid(const float* x, float* y, int64_t n, sd_stream_t stream);

/* nms, utils.py:441-443: out = (hm == maxpool5x5(hm)) * hm, -inf padding.  in strided
 * (sb, sc), out contiguous (B,C,h,w).  apply_sigmoid != 0 fuses clamped_sigmoid first. */
int sd_nms5(const float* hm, int64_t sb, int64_t sc, float* out, int B, int C, int h, int w,
            int apply_sigmoid, sd_stream_t stream);

/* topk, utils.py:447-467 on an arbitrary (B,C,h,w) score map (no sigmoid, no NMS): global top-k
 * over the class-major flattened map; order: score desc, class asc, flat index asc.
 * Outputs (B,k): score f32, ind i64, cls f32, ys f32, xs f32. */
size_t sd_topk_workspace_bytes(int B, int C, int h, int w, int k);
int sd_topk(const float* scores, int64_t sb, int64_t sc, int B, int C, int h, int w, int k,
            float* out_score, int64_t* out_ind, float* out_cls, float* out_ys, float* out_xs,
            void* workspace, size_t workspace_bytes, sd_stream_t stream);

/* transpose_and_gather, utils.py:347-351: feat (B,C,h*w) strided, ind (B,n) i64 -> out (B,n,C). */
int sd_transpose_and_gather(const float* feat, int64_t sb, int64_t sc, int B, int C, int64_t hw,
                            const int64_t* ind, int n, float* out, sd_stream_t stream);

/* hypot, utils.py:422-437: out[i] = sqrt(fl(fl(x0*x0) + fl(x1*x1))) over n pairs (no FMA). */
int sd_hypot(const float* in_pairs, float* out, int64_t n, sd_stream_t stream);

/* ---- decoder: src/sdnet/data/decoders.py:29-179 ------------------------------------------- */

/* D1-D3 (decoders.py:44-48 / 60-64): clamped sigmoid + 5x5 NMS + top-k of one heatmap group,
 * fused (logits are read once).  Same outputs as sd_topk. */
size_t sd_decode_peaks_workspace_bytes(int B, int C, int h, int w, int k);
int sd_decode_peaks(const float* logits, int64_t sb, int64_t sc, int B, int C, int h, int w, int k,
                    float* out_score, int64_t* out_ind, float* out_cls, float* out_ys, float* out_xs,
                    void* workspace, size_t workspace_bytes, sd_stream_t stream);

/* Whole device stage of Decoder.__call__ (decoders.py:41-100) in two launches (+1 memset node):
 * peaks of the anchor group (M maps, top K) and of the part group (N maps, top P), offset /
 * embedding gather, refinement, masking, K x P association.
 * `packed` receives B*(6K+11P) 4-byte words, structure-of-arrays over the batch:
 *   anchor_out   f32 (B,K,4)  x, y, raw score, label           decoders.py:55-57
 *   part_out     f32 (B,P,6)  x, y, raw score, kind, ox, oy    decoders.py:72-75
 *   part_emb     f32 (B,P,2)                                   decoders.py:66
 *   anchor_smask f32 (B,K)    score, or -1 where score <= conf  decoders.py:84
 *   part_smask   f32 (B,P)                                     decoders.py:79
 *   anchor_ind   i32 (B,K)    flat y*w+x                        decoders.py:46
 *   part_ind     i32 (B,P)
 *   assign       i32 (B,P)    anchor rank, or -1 when min dist >= dist_px  decoders.py:98-100
 *   status       i32 (B)      0 = ok; 1 = sd_decode_fused gave up waiting for a tile block (that image's results are invalid)
 * conf and dist_px are the fp32-rounded thresholds.
 * exact_topk = 1: every slot equals the reference's top-k, including peaks below conf (needed by return_metadata=True);
 * exact_topk = 0: peaks with score <= conf are dropped at compaction -- the assembled annotations are identical (the
 * reference skips / masks those entries, decoders.py:78-86,115-117) and the selection has far fewer candidates to sort;
 * slots past the surviving peaks are then zero-score fillers. */
size_t sd_decode_workspace_bytes(int B, int M, int N, int h, int w, int K, int P);
size_t sd_decode_packed_words(int B, int K, int P);
int sd_decode(const float* anchor_hm, int64_t a_sb, int64_t a_sc,
              const float* part_hm, int64_t p_sb, int64_t p_sc,
              const float* offsets, int64_t o_sb, int64_t o_sc,
              const float* embeddings, int64_t e_sb, int64_t e_sc,
              int B, int M, int N, int h, int w, int K, int P, float conf, float dist_px, int exact_topk,
              void* packed, void* workspace, size_t workspace_bytes, sd_stream_t stream);

/* The same decoder in ONE launch (no second kernel, no memset): the last tile block to arrive for an image runs the selection
 * and association for it.  Results are bit-identical to sd_decode.  max_objects and max_parts up to 512, B up to 256.
 * `state`: sd_decode_state_bytes(B) bytes of device memory owned by the caller and used by nothing else, which must be ZERO
 * before the first call; every call leaves it zero again (so back-to-back calls and hipGraph replays need no memset).  After a
 * failed or aborted launch re-zero it.  `workspace`: sd_decode_fused_workspace_bytes() bytes of scratch (per-tile candidate
 * slots and counts; contents need no initialisation).  Images whose (M+N) x tiles bookkeeping does not fit 64 KB of LDS
 * (e.g. 2048x2048 inputs with 16 maps) are rejected with SD_ERR_INVALID: use sd_decode for those.
 * Replaces decoders.py:41-100 like sd_decode; exists because bs = 1 inference is launch-latency-bound. */
size_t sd_decode_state_bytes(int B, int M, int N, int h, int w);
int    sd_decode_fused_supported(int B, int M, int N, int h, int w, int K, int P);   /* 1 when sd_decode_fused can compute this geometry */
/* 1 where ONE launch is also the FASTER decoder (at most 256 tile blocks per image: 512x512 with 2 + 1 maps has 48; exact top-k: batches
 * up to 8).  Elsewhere call sd_decode: at 1024x1024 / 8 + 8 maps / K = 128 / P = 512 the one-launch form takes 451 us against 116 us.
 * sd_decode_fused REFUSES (SD_ERR_INVALID) image geometries beyond 256 tile blocks unless bit 1 of `exact_topk` (value 2) is set. */
int    sd_decode_fused_recommended(int B, int M, int N, int h, int w, int K, int P, int exact_topk);
size_t sd_decode_fused_workspace_bytes(int B, int M, int N, int h, int w, int K, int P);
int sd_decode_fused(const float* anchor_hm, int64_t a_sb, int64_t a_sc,
                    const float* part_hm, int64_t p_sb, int64_t p_sc,
                    const float* offsets, int64_t o_sb, int64_t o_sc,
                    const float* embeddings, int64_t e_sb, int64_t e_sc,
                    int B, int M, int N, int h, int w, int K, int P, float conf, float dist_px, int exact_topk,
                    void* packed, void* state, size_t state_bytes, void* workspace, size_t workspace_bytes, sd_stream_t stream);
/* A/B and test switches of the two decoders (none changes a result; THREAD-LOCAL: a value applies to calls made by the host thread
 * that set it, every thread starts from the defaults, so two engines in two threads of one process cannot disturb each other).
 * Unknown names: SD_ERR_INVALID.  The keys, in the order of the table in csrc/sd_decode.hip (INTEGRATION.md has the same list):
 *   "tall_tiles_from" (2688)   sd_decode_fused: number of 64x16-pixel tile blocks of a launch (B x (M+N) x tiles) from which the NMS runs
 *                              on 64x32 tiles instead (batches of 56 and more at 128x128 maps; 1 = always, 1 << 30 = never).  The sizes
 *                              returned by sd_decode_state_bytes / _workspace_bytes cover both.
 *   "map_parallel_from" (-1)   sd_decode: number of 64x16-pixel tile blocks of a call from which it takes its map-parallel path -- tile
 *                              pass without global atomics, one selector block per (image, map) or part of a map, one merge + association
 *                              block per image; bit-identical results -- instead of the launch pair with one selector block per image.
 *                              -1 = by geometry and mode: on maps up to 128 columns wide sd_decode always takes it, and the one-launch
 *                              kernel is recommended below 960 tile blocks without the exact top-k only; wider maps from 2560; always for
 *                              images of 1024+ tile blocks such as 1024x1024 inputs with 8 + 8 maps; sd_decode_fused_recommended follows
 *                              the same rule.  A value >= 0 holds for every geometry and mode: 1 = always, 1 << 30 = never.
 *   "map_rows11" (1)           bands of 128-row maps in k_map_stream_select: 1 = 8-row bands with two bands per wave on launches of
 *                              fewer than 1024 maps, else 11-row bands; 0 = 16-row bands; 8 / 11 = forced.
 *   "map_stream" (1)           0 = tile kernel + k_select_map instead of k_map_stream_select inside the map-parallel path.
 *   "map_tile_height" (0)      rows per NMS tile of that tile kernel: 16 / 32 / 0 (by size).
 *   "map_scalar_nms" (0)       1 = the per-pixel-sigmoid tile kernel also where the logit-domain one (w % 4 == 0, aligned planes) applies.
 *   "map_split" (0)            blocks of k_map_stream_select per map: 0 = by size, 1 .. 4 = forced.
 *   "map_half" (1)             0 = one band per wave also on maps up to 128 columns wide (1: two bands per wave there).
 *   "map_waves3" (1)           parts of three wave-iterations of work on 192-thread blocks: 1 = from 1024 blocks per launch when a score
 *                              threshold keeps the selections short, 0 = never, 2 = always.
 *   "map_rank_group" (1)       ranks + gathers + association of an image: 1 = by size (k_rank_group_small, k_rank_group<256>, else
 *                              k_rank_maps + k_group_wide), 0 = always the pair, 2 = the one-block kernel wherever its lists fit LDS. */
int sd_decode_set_option(const char* name, int value);
/* What a decode would launch, for the CALLING thread's options (host arithmetic only, no HIP call; profiling labels and dispatch tables:
 * tools/decode_dispatch_table.py).  flags bit 0: the heat-map planes are vector-loadable (16-byte aligned base pointers, strides that are
 * multiples of 4 floats); bit 1: describe sd_decode_fused (exact_topk with its override bit) instead of sd_decode (annotations-only is
 * planned with a positive confidence threshold).  One line: each launch as "<kernel as rocprofv3 prints it, without sd::> grid=XxYxZ
 * block=T lds=<dynamic LDS bytes>", launches in order, separated by "; "; the counter memset of the launch pair is listed as "memset";
 * "refused: <message>" where sd_decode_fused would return an error; "" for a non-positive argument.  Thread-local storage, valid until
 * the next call on the thread. */
const char* sd_decode_kernel_names(int B, int M, int N, int h, int w, int K, int P, int exact_topk, int flags);

/* Device self-check of the two properties the logit-domain NMS tile pass of sd_decode rests on, over ALL 2^32 fp32 bit patterns:
 * out3[0] = violations of "clamped sigmoid is monotone non-decreasing", out3[1] = violations of the near-tie margin table
 * (a logit further below the window maximum than the margin has a strictly smaller sigmoid), out3[2] = values visited
 * (2^32 - NaNs = 4 278 190 082).  out3: three 64-bit words of device memory.  ~10 ms. */
int sd_selfcheck_sigmoid(unsigned long long* out3, sd_stream_t stream);

/* Explicit host wait for everything queued on `stream` (hipStreamSynchronize): the ONE blocking call of the decoder's host side,
 * after which a `packed` buffer that lives in pinned, device-mapped host memory may be read (decoders.py:103-139 reads its
 * tensors through ~200 implicit synchronisations instead).  No other function of this library blocks. */
int sd_stream_synchronize(sd_stream_t stream);

/* D4-D5 alone (decoders.py:49-100) from already selected peaks (outputs of sd_decode_peaks):
 * same `packed` layout as sd_decode. */
int sd_decode_group(const float* a_score, const int64_t* a_ind, const float* a_cls,
                    const float* p_score, const int64_t* p_ind, const float* p_cls,
                    const float* offsets, int64_t o_sb, int64_t o_sc,
                    const float* embeddings, int64_t e_sb, int64_t e_sc,
                    int B, int h, int w, int K, int P, float conf, float dist_px,
                    void* packed, sd_stream_t stream);

/* ---- flip test-time augmentation (no reference counterpart: the reference decodes one forward of the unflipped image) ----
 * `view_flips_host` is a HOST array of V bytes, one per view: bit 0 = horizontal, bit 1 = vertical flip (the encoding of
 * sd_preprocess_images' `flips`).  V is 2 or 4 and view 0 must be the unflipped image (byte 0); anything else is SD_ERR_INVALID.
 * Both functions are one launch each, use no workspace and no atomics, and are deterministic.
 *
 * sd_tta_views: x (B,3,H,W) fp32 NCHW contiguous -> out (V*B,3,H,W); view v of image b is image v*B + b of `out`:
 *   out[v*B + b, c, y, x] = x[b, c, fy(y), fx(x)],  fy(y) = H-1-y if bit 1 of view v else y,  fx(x) = W-1-x if bit 0 else x.
 *   The input is read once; every view -- mirrored rows too -- is written as contiguous spans.
 *
 * sd_tta_merge_nms: `hm` = the heatmap logits of a head output of V*B images ordered as above, a strided (sb, sc) channel-slice view
 *   like every other map argument; out (B,C,h,w) contiguous.  For every pixel
 *       m(y, x) = (s_0 + s_1 [+ s_2 + s_3]) * (1/V),   s_v = clamped_sigmoid(hm[v*B + b, c, fy_v(y), fx_v(x)])
 *   -- the device function behind sd_clamped_sigmoid, the terms added in view order v = 0 .. V-1 in fp32, each add and the final multiply
 *   rounded separately (no FMA contraction) -- and out = m where m equals the maximum of m over the 5x5 window, else 0; padding (-inf)
 *   and ties exactly as sd_nms5.  Equal, bit for bit, to sd_nms5 of that sum formed from sd_clamped_sigmoid outputs.  Every view's logits
 *   are read once and the output is written once; 16-byte loads when w % 4 == 0 and planes / strides are 16-byte aligned, 4-byte loads
 *   otherwise. */
int sd_tta_views(const float* x, float* out, int B, int H, int W, int V, const unsigned char* view_flips_host, sd_stream_t stream);
int sd_tta_merge_nms(const float* hm, int64_t sb, int64_t sc, float* out, int B, int C, int h, int w, int V,
                     const unsigned char* view_flips_host, sd_stream_t stream);

/* ---- multi-scale test-time augmentation (no reference counterpart) ----
 * sd_tta_scale_merge_nms: the heatmap logits of S forwards at S input sizes, each over V mirrored views, merged on the base grid:
 *   scale s is a (V*B, C, hs[s], ws[s]) strided (sb[s], sc[s]) channel-slice view at hm_host[s] (device pointers; the five arrays
 *   `*_host` are HOST arrays of S entries), view v of image b is image v*B + b as in sd_tta_views; out (B,C,h,w) contiguous.
 *   1 <= S <= 5, V in {1, 2, 4}, view 0 unflipped, 1 <= hs[s] <= 2h and 1 <= ws[s] <= 2w (the bound that fits the source footprint
 *   of a 64x16 tile and its halo, <= 138 x 42 cells, into LDS); anything else is SD_ERR_INVALID.  Scale 0 need not be the base size.
 *   One launch, no workspace, no atomics, no host synchronisation, deterministic.  For base cell (y, x), with all coordinate
 *   arithmetic in double and every fp32 operation rounded separately (no contraction):
 *       rx = (double)ws / (double)w;  sx = max((x + 0.5) * rx - 0.5, 0);  x0 = min((int)floor(sx), ws-1);  x1 = min(x0 + 1, ws-1);
 *       lx = sx - x0;  wx1 = (float)lx;  wx0 = (float)(1.0 - lx)        (the vertical axis alike: torch's bilinear, align_corners=False)
 *       p_v(yy, xx) = clamped_sigmoid(hm_s[v*B + b, c, fy_v(yy), fx_v(xx)]),  fx_v(xx) = ws-1-xx if bit 0 of view v else xx, fy_v alike
 *       top = wx0 * p_v(y0, x0) + wx1 * p_v(y0, x1);  bot = wx0 * p_v(y1, x0) + wx1 * p_v(y1, x1);  r_{s,v} = wy0 * top + wy1 * bot
 *       m = (sum of r_{s,v}, scale-major, view-minor, from r_{0,0}) * inv,   inv = the fp32 nearest to the double 1.0 / (S * V)
 *   and out = m where m equals the maximum of m over the 5x5 window, else 0; padding and ties exactly as sd_nms5.  Equal sizes give
 *   x0 = x, wx0 = 1, wx1 = 0: with S = 1 at the base size the function equals sd_tta_merge_nms bit for bit (and runs its kernel), and
 *   with V = 1 as well sd_nms5(apply_sigmoid = 1).  Every source cell's sigmoid is computed once per block; every view is read once
 *   (+ halo re-reads), the output written once; 16-byte loads per scale when ws % 4 == 0 and planes / strides are 16-byte aligned,
 *   4-byte loads otherwise. */
int sd_tta_scale_merge_nms(const float* const* hm_host, const int64_t* sb_host, const int64_t* sc_host, const int* hs_host,
                           const int* ws_host, float* out, int B, int C, int h, int w, int S, int V,
                           const unsigned char* view_flips_host, sd_stream_t stream);

/* ---- transposed views (no reference counterpart): the four symmetries of the grid that the flips do not reach ----
 * `view_flips_host` is a HOST array of Vf bytes in the encoding of sd_tta_views, Vf in {1, 2, 4}, byte 0 must be 0 and every byte < 4.
 * All three functions validate every argument on the host before any launch (anything else is SD_ERR_INVALID), are one launch each, use no
 * workspace, no atomics and no host synchronisation, and are deterministic.  Every transposed plane is staged through LDS tiles of an odd
 * dword pitch, so global loads and stores both run along the fast axis; 16-byte accesses where pointer and row length allow, 4-byte ones
 * otherwise.
 *
 * sd_d4_views: x (B,3,H,W) fp32 NCHW contiguous -> out (Vf*B,3,H,W) and out_t (Vf*B,3,W,H); view v of image b is image v*B + b of both:
 *       out  [v*B + b, c, y, x] = x[b, c, fy(y), fx(x)]          -- exactly what sd_tta_views writes
 *       out_t[v*B + b, c, r, s] = xT[b, c, fy'(r), fx'(s)],  xT[b, c, r, s] = x[b, c, s, r]   -- transpose FIRST, then flip the transposed image:
 *   fy'(r) = W-1-r if bit 1 of view v else r, fx'(s) = H-1-s if bit 0 else s.  With H == W, out_t = out + Vf*B*3*H*W makes the two one
 *   batch of 2*Vf*B images.  The input is read once.
 *
 * sd_d4_merge_nms: `hm` = heatmap logits of the plain views, a strided (sb, sc) channel-slice view of (Vf*B, C, h, w); `hm_t` = those of
 *   the transposed views, (Vf*B, C, w, h) with strides (sb_t, sc_t); out (B,C,h,w) contiguous.  With s_v(y, x) = clamped_sigmoid(hm[v*B + b, c,
 *   fy_v(y), fx_v(x)]) as in sd_tta_merge_nms and t_v(y, x) = clamped_sigmoid(hm_t[v*B + b, c, fy'_v(x), fx'_v(y)]) (the flipped transposed map,
 *   transposed back),
 *       m = ((s_0 [+ s_1 [+ s_2 + s_3]]) + (t_0 [+ t_1 [+ t_2 + t_3]])) * (1 / (2 Vf))
 *   -- each sum from its view 0 in view order, then the two sums added, in fp32, every add and the multiply rounded separately -- and out = m
 *   where m equals the maximum of m over the 5x5 window, else 0; padding and ties exactly as sd_nms5.
 *
 * sd_transpose_select: x, out (B,P,S,S) fp32 contiguous, not overlapping (refused); `sel_dev` a DEVICE table of B bytes: image b of out is
 *   the transpose of image b of x where sel_dev[b] & 1, a copy otherwise (the other bits are masked). */
int sd_d4_views(const float* x, float* out, float* out_t, int B, int H, int W, int Vf, const unsigned char* view_flips_host,
                sd_stream_t stream);
int sd_d4_merge_nms(const float* hm, int64_t sb, int64_t sc, const float* hm_t, int64_t sb_t, int64_t sc_t, float* out, int B, int C, int h,
                    int w, int Vf, const unsigned char* view_flips_host, sd_stream_t stream);
int sd_transpose_select(const float* x, float* out, int B, int P, int S, const unsigned char* sel_dev, sd_stream_t stream);

/* ---- evaluation matching (no reference counterpart: the reference matches on the host, at one confidence threshold) ----
 * Labels EVERY top-k slot of a decoded batch a hit or a miss against the ground truth, the way the Evaluator matches anchors and raw parts
 * (greedy by descending score; a prediction only ever tries its nearest ground truth of its class).  Whether slot i is a hit depends only
 * on the slots ranked above it, so the counters at ANY confidence threshold are prefix counts over the slots the threshold keeps.
 *   a_list (B,K,4) fp32, words x, y, score, class: the anchor_out part of sd_decode's `packed`;  p_list (B,P,6) fp32, same first four words:
 *   its part_out part.  1 <= K, P <= SD_MAX_TOPK.  Both lists are in score-descending order, as sd_decode writes them (not checked).
 *   gt_xy (G,2) fp64: every ground-truth point of the batch in SOURCE-IMAGE pixels;  gt_cls (G) int32: their classes (negative: matches
 *   nothing);  gt_off (2B+1) int32: segment b = [gt_off[b], gt_off[b+1]) holds the anchors of image b, segment B + b its parts (device
 *   data: the kernel clamps every offset into [0, G], so any table is memory-safe);  G >= 0 (the pointers are needed even then).
 *   img (B,3) fp64: per image fx, fy, thr;  sx, sy: cell -> network-input pixel scale.
 *   match, dist: (B, K+P) int32 / fp64; row b holds the K anchor slots, then the P part slots.
 * For slot i of a list with segment S, in fp64 with every operation rounded separately (no contraction):
 *       X = ((double)x * sx) * fx;   Y = ((double)y * sy) * fy;   d_j = hypot(X - gx_j, Y - gy_j)  over the j of S with gt_cls[j] == (int)class
 *       j* = the first minimum (lowest j on equal distance);  dist = d_j*, or +inf when S has no ground truth of that class
 *       match = j* - gt_off[S]  when d_j* < thr (strictly) AND i is the lowest slot index of its list with that j* and a distance below thr,
 *               else -1 (a prediction gets no second choice).
 * All slots are matched whatever their score: a filler slot has a higher index than every real one and cannot displace it.
 * One launch (one 256-thread block per image and list; the ground truths pass through LDS SD_EVAL_GT_CHUNK at a time), no workspace, no
 * host synchronisation, integer LDS atomics only: deterministic.  Null pointers, non-positive B / K / P, K or P beyond SD_MAX_TOPK and a
 * negative G: SD_ERR_INVALID; a_list / gt_xy not 16-byte, p_list / img / dist not 8-byte, the int32 tables not 4-byte aligned: SD_ERR_ALIGN. */
#define SD_EVAL_GT_CHUNK 1024
int sd_eval_match(const float* a_list, const float* p_list, int B, int K, int P, const double* gt_xy, const int* gt_cls, const int* gt_off,
                  int G, const double* img, double sx, double sy, int* match, double* dist, sd_stream_t stream);

/* ---- tiled inference (no reference counterpart: the reference resizes the whole image to one network input) ----
 * A canvas of Wc = Tx*W - (Tx-1)*O by Hc = Ty*H - (Ty-1)*O pixels is cut into Ty x Tx overlapping tiles of the network's own input size
 * W x H; tile (j, i) starts at pixel (j*(H-O), i*(W-O)); tile t = j*Tx + i of image b is image t*B + b (the ordering of sd_tta_views).
 * 1 <= Tx, Ty <= 8 and 0 <= 2*O <= min(H, W) (at most two tiles cover a cell along an axis); all geometry is validated on the host
 * before any HIP call, anything else is SD_ERR_INVALID.  Both functions are one launch each, use no workspace, no atomics and no host
 * synchronisation, and are deterministic.
 *
 * sd_tile_views: canvas (B,3,Hc,Wc) fp32 NCHW contiguous -> out (Ty*Tx*B,3,H,W):
 *       out[t*B + b, c, y, x] = canvas[b, c, j*(H-O) + y, i*(W-O) + x].
 *   Requires Wc == Tx*W - (Tx-1)*O and Hc == Ty*H - (Ty-1)*O.  16-byte accesses when W, O and Wc are multiples of 4 and the pointers
 *   are 16-byte aligned, 4-byte accesses otherwise.
 *
 * sd_tile_merge_nms: all sizes in cells.  `hm` = the heatmap logits of the T*B tile forwards, a strided (sb, sc) (T*B, C, h, w)
 *   channel-slice view; `reg` a strided (r_sb, r_sc) (T*B, R, h, w) view of the regression channels (offsets + embeddings; R = 0 with
 *   null pointers is allowed).  out_hm (B,C,hc,wc) and out_reg (B,R,hc,wc) contiguous, wc = Tx*w - (Tx-1)*o, hc = Ty*h - (Ty-1)*o.
 *   Per axis, shown for x (y alike): for canvas column X, i_hi = min(X / (w-o), Tx-1) and l = X - i_hi*(w-o).  If i_hi > 0 and l < o two
 *   tiles cover the column: tile i_hi-1 at local column l + (w-o) with weight w_lo = (float)((double)(o-l) / (double)(o+1)), and tile
 *   i_hi at local column l with weight w_hi = (float)((double)(l+1) / (double)(o+1)).  Otherwise only tile i_hi covers it, weight 1.0f.
 *   Heatmaps: for every covering tile in ascending t order (row-major)  p = clamped_sigmoid(logit) -- the device function behind
 *   sd_clamped_sigmoid --, wt = wy * wx, c = wt * p; m = the sum of the c in that order, every fp32 operation rounded separately;
 *   out_hm = m where m equals the 5x5 maximum of m over the canvas, else 0: seams get no special treatment, padding (-inf) and ties
 *   exactly as sd_nms5.  Regressions: out_reg is a bit copy from the owner tile; per axis the owner is the covering tile with the
 *   larger weight, the lower-index tile on a tie (o odd, l = (o-1)/2).  Offsets are sub-cell and embeddings displacements in cells:
 *   both are translation-invariant and need no correction.
 *   Consequences: Tx = Ty = 1 equals sd_nms5(apply_sigmoid = 1) bit for bit; o = 0 equals sd_nms5 of the concatenated tile maps; every
 *   cell covered by a single tile keeps its probability unchanged.  16-byte loads when w and o are multiples of 4 and planes / strides
 *   are 16-byte aligned, 4-byte loads otherwise. */
int sd_tile_views(const float* canvas, float* out, int B, int Hc, int Wc, int H, int W, int Ty, int Tx, int O, sd_stream_t stream);
int sd_tile_merge_nms(const float* hm, int64_t sb, int64_t sc, int C, const float* reg, int64_t r_sb, int64_t r_sc, int R,
                      float* out_hm, float* out_reg, int B, int h, int w, int Ty, int Tx, int o, sd_stream_t stream);

/* ---- cross-label anchor suppression (no reference counterpart: the reference suppresses per heatmap channel only) ----
 * sd_label_nms: `p` = P, the per-label suppressed probability maps (what sd_nms5(apply_sigmoid = 1) or a merge kernel writes), a strided
 *   (sb, sc) (B,M,h,w) view (for example the anchor slice of a merge kernel's output); out (B,M,h,w) contiguous; R = the radius in cells.
 *   Per image:
 *       best(y, x)  = max over c < M of P[c, y, x];      first(y, x) = the lowest c with P[c, y, x] == best(y, x)
 *       win(y, x)   = max of best over |dy| <= R, |dx| <= R; cells outside the map do not count (-inf padding)
 *       out[c, y, x] = P[c, y, x] if P[c, y, x] == win(y, x) and c == first(y, x), else 0
 *   Only max and ==: equal values at different cells inside a window both survive (as in sd_nms5), a tie of labels at one cell goes to the
 *   lowest label, and the rule is one max-pool, not a greedy loop: a peak suppressed by a neighbour still suppresses.  With M = 1 and
 *   R <= 2 the output equals the input; with R > 2 peaks of one label closer than R are thinned as well.
 *   1 <= R <= 8, 1 <= M <= 256, B <= 65535, M*h*w < 2^31, sb and sc >= h*w, no null pointer; anything else is SD_ERR_INVALID.  One launch,
 *   no workspace, no atomics, no host synchronisation, deterministic.  One block per 64x16 tile and image walks the M label planes, each
 *   read once (+ halo re-reads), and writes every label plane of its tile from registers; 16-byte accesses when w % 4 == 0 and pointers /
 *   strides are 16-byte aligned, 4-byte accesses otherwise, same result. */
int sd_label_nms(const float* p, int64_t sb, int64_t sc, float* out, int B, int M, int h, int w, int R, sd_stream_t stream);

/* ---- target rendering: src/sdnet/data/transforms.py:130-205 (Encode) ---------------------- */

/* Heatmaps of a batch (transforms.py:143,160-161,173-174; utils.py:418-419): for every pixel of
 * channel c of image b, exp(fp32(-min d^2) / two_sigma2) over that channel's keypoint centres,
 * 0 when the channel has none.  Centres are the truncated output-pixel coordinates
 * (cx[i], cy[i]) sorted by (image, channel); chan_ptr (B*C+1) is the CSR row pointer.
 * out: (B,C,h,w) contiguous fp32. */
int sd_render_targets(const int32_t* cx, const int32_t* cy, const int32_t* chan_ptr,
                      int B, int C, int h, int w, float two_sigma2, float* out, sd_stream_t stream);

/* ---- input pipeline: src/sdnet/data/transforms.py:9-35,47-60,108-118 (flips, Resize, Normalize) ------------------------ */

/* The preprocess chain, one call per batch, every image operation byte for byte Pillow's (or the stated integer definition):
 *     Resize | Window | Letterbox -> [Mosaic] -> [Affine | Perspective] -> [Blur] -> [Noise] -> [JPEG] -> [Tone] -> [ColorJitter]
 *     -> flips -> to_tensor -> Normalize            (transforms.py:217-226 order; out: (B, 3, Hout, Wout) fp32 NCHW)
 * sd_preprocess_chain is the entry point for new callers; every stage in brackets is a table of the descriptor that is null when off.
 *
 * Source.  images: (B, Hin, Win, 3) u8 on the device, or with list != 0 a DEVICE array of B device pointers, each to one (Hin, Win, 3)
 *   u8 image, any byte alignment, duplicates allowed (a cache of decoded images).  The list form stages source rows in LDS: Win (with a
 *   window: g1) <= 21834, SD_ERR_INVALID beyond.  The two forms give the same bytes.
 * Resize.  PIL bilinear: Pillow's 22-bit fixed-point separable resampling, horizontal pass first.  h_bounds / h_kk (per output column
 *   {first source column, count} and h_ksize fixed-point weights) and v_bounds / v_kk (per output row) are the tables of Pillow's
 *   precompute_coeffs + normalize_coeffs_8bpc, made by the host (data/augment.py) and resident on the device.  geometry:
 *     SD_GEOM_STRETCH    tables Win -> Wout, Hin -> Hout; Hg, Wg, g0, g1 are not read and window is null.
 *     SD_GEOM_WINDOW     crop training: image b's resize target is the (Hg, Wg) canvas (tables Win -> Wg, Hin -> Hg) of which only the
 *                        (Hout, Wout) window at window[b] = (x0, y0) -- (B, 2) int32 on the device, clamped into the canvas by the
 *                        kernels -- is produced: Image.resize((Wg, Hg)).crop(...).  g0 = max_rows, g1 = max_cols: HOST upper bounds of
 *                        any window's source row / column span (data/augment.py window_extents), in [1, Hin] / [1, Win]; only those
 *                        rows and columns are read.  A window larger than the canvas or a null table is SD_ERR_INVALID.
 *     SD_GEOM_LETTERBOX  aspect-preserving input: the source is resized to (Hg, Wg) (tables Win -> Wg, Hin -> Hg) and pasted at
 *                        (x0, y0) = (g1, g0) into a (Hout, Wout) frame of fill3, which is always needed; an image that does not lie
 *                        inside the frame is SD_ERR_INVALID.  window is null.
 *   Every later stage works on the (Hout, Wout) result; grey means and histograms include fill pixels and bars.
 * Mosaic.  mosaic_geom (B, 6) int32 = cx, cy, s0 .. s3 and mosaic_affine (B, 4, 6) fp64, both or neither: output pixel (x, y) lies in
 *   quadrant q = (x >= cx) + 2 (y >= cy) and takes Image.transform(AFFINE, m_q, BILINEAR, fillcolor = fill3) of resized image s_q of THIS
 *   batch.  The kernels clamp cx, cy and s_q: any table is memory-safe.  A row (Wout, Hout, b, -, -, -) with m_0 the identity copies b.
 * Warp.  affine (B, 6) fp64 = the inverse matrix [m0 .. m5] that maps an output pixel centre (x + 0.5, y + 0.5) to the source position
 *   (m0 x + m1 y + m2, m3 x + m4 y + m5), Image.transform(AFFINE, ..., BILINEAR, fillcolor = fill3); or persp (B, 8) fp64 as
 *   sd_perspective_u8's coefficients.  Not both (SD_ERR_INVALID: fold the affine matrix into the homography).  A warp or a mosaic needs
 *   fill3 (HOST pointer to three bytes).
 * Blur, Noise, JPEG, Tone.  blur (B, 3), noise (B, 4), jpeg (B, 129), tone (B, 4) int32 on the device: the tables of sd_blur_u8,
 *   sd_noise_u8, sd_jpeg_u8 and sd_tone_u8 below, the same bytes.  jpeg needs Hout and Wout multiples of 16; jpeg and tone need a
 *   16-byte aligned workspace; noise and tone need Hout * Wout < 2^31.
 * ColorJitter.  torchvision ColorJitter on the 8-bit image (ImageEnhance.Brightness / Contrast / Color and the HSV round trip of
 *   adjust_hue).  jitter_order (B) int32: bits 0-7 = the four op ids in application order, 2 bits each (0 brightness, 1 contrast,
 *   2 saturation, 3 hue), bits 8-15 = the hue shift byte uint8(hue_factor * 255); jitter_factors (B, 3) fp32; both or neither.
 * flips: B bytes (bit 0 = horizontal, bit 1 = vertical) or null.  mean3 / std3: HOST pointers to three floats.  The draws are the caller's.
 *
 * Launches.  H and V are the geometry's horizontal and vertical kernels; "late" = persp, blur, noise, jpeg or tone is set; with jitter
 * a memset of the grey sums comes first.  A and B are the workspace's two 8-bit images.
 *     none                      H, V_norm -> out             mosaic                    H, V -> B, mosaic_norm -> out
 *     jitter                    H, V -> A, J                 mosaic + jitter           H, V -> B, mosaic -> A, J
 *     affine                    H, V -> B, affine_norm -> out  mosaic + affine         H, V -> A, mosaic -> B, affine_norm -> out
 *     affine + jitter           H, V -> B, affine -> A, J    mosaic + affine + jitter  H, V -> A, mosaic -> B, affine -> A, J
 *     late: H, V, [mosaic], [affine | persp] alternating so that the last writes A, [blur A -> B -> A], [noise], [jpeg], [tone] on A in
 *           place, then J or k_u8_norm -> out                (J = k_jitter_lsum + k_jitter_norm -> out)
 * sd_preprocess_kernel_names prints the plan of a descriptor: the launches in order, separated by "; ", each as
 * "<kernel> grid=XxYxZ block=256 lds=N dst=tmp|A|B|out|sums", "memset", the late stages as "blur", "noise", "jpeg", "tone", or
 * "refused: <message>" where the chain would return an error (thread-local storage; sets sd_last_error then).
 *
 * workspace: [horizontal intermediate | image A | grey sums | image B | JPEG planes | tone histograms], each a multiple of 256 bytes;
 * sd_preprocess_chain_workspace_bytes() (0 for a descriptor the chain refuses) is the end of the last region the plan uses -- the
 * intermediate for the plain stretch, the grey sums for the stretch with jitter alone, image B otherwise (the window and letterbox
 * geometries always reserve up to there), the planes with jpeg, the histograms (behind the planes' place) with tone.  A short workspace
 * is SD_ERR_WORKSPACE.
 * Limits.  B <= 65535 when jitter, a warp, a mosaic or a late stage is set (B is a grid dimension there), Hout <= 65535 * 64 with a late
 * stage; no batch limit on the plain resize. */
#define SD_GEOM_STRETCH   0
#define SD_GEOM_WINDOW    1
#define SD_GEOM_LETTERBOX 2
typedef struct sd_preprocess_desc {
    const void* images; int list;
    int geometry;
    int B, Hin, Win, Hg, Wg, Hout, Wout, g0, g1;
    const int *h_bounds, *h_kk; int h_ksize; const int *v_bounds, *v_kk; int v_ksize;
    const int* window; const uint8_t* flips; const int* jitter_order; const float* jitter_factors;
    const double *affine, *persp; const int* mosaic_geom; const double* mosaic_affine;
    const int *blur, *noise, *jpeg, *tone;
    const uint8_t* fill3; const float *mean3, *std3; float* out;
} sd_preprocess_desc;
size_t sd_preprocess_chain_workspace_bytes(const sd_preprocess_desc* d);
int sd_preprocess_chain(const sd_preprocess_desc* d, void* workspace, size_t workspace_bytes, sd_stream_t stream);
const char* sd_preprocess_kernel_names(const sd_preprocess_desc* d);

/* The entry points from before the descriptor, kept for their callers: each is sd_preprocess_chain on the fields it names (the stages it
 * has no argument for are off; a null table is the form below it, bit for bit), with errors under its own name.  The *_workspace_bytes
 * functions give the chain's layout with every region of their form. */
/* Resize -> flips -> Normalize.  workspace: the horizontal intermediate. */
size_t sd_preprocess_workspace_bytes(int B, int Hin, int Win, int Wout);
int sd_preprocess_images(const uint8_t* images, int B, int Hin, int Win, int Hout, int Wout,
                         const int* h_bounds, const int* h_kk, int h_ksize, const int* v_bounds, const int* v_kk, int v_ksize,
                         const uint8_t* flips, const float* mean3, const float* std3, float* out,
                         void* workspace, size_t workspace_bytes, sd_stream_t stream);
int sd_preprocess_images_list(const uint8_t* const* images, int B, int Hin, int Win, int Hout, int Wout,
                              const int* h_bounds, const int* h_kk, int h_ksize, const int* v_bounds, const int* v_kk, int v_ksize,
                              const uint8_t* flips, const float* mean3, const float* std3, float* out,
                              void* workspace, size_t workspace_bytes, sd_stream_t stream);
/* ... with ColorJitter: both jitter tables are required.  workspace: up to the grey sums. */
size_t sd_preprocess_jitter_workspace_bytes(int B, int Hin, int Win, int Hout, int Wout);
int sd_preprocess_images_jitter(const uint8_t* images, int B, int Hin, int Win, int Hout, int Wout, const int* h_bounds, const int* h_kk,
                                int h_ksize, const int* v_bounds, const int* v_kk, int v_ksize, const uint8_t* flips, const int* jitter_order,
                                const float* jitter_factors, const float* mean3, const float* std3, float* out, void* workspace,
                                size_t workspace_bytes, sd_stream_t stream);
int sd_preprocess_images_list_jitter(const uint8_t* const* images, int B, int Hin, int Win, int Hout, int Wout, const int* h_bounds,
                                     const int* h_kk, int h_ksize, const int* v_bounds, const int* v_kk, int v_ksize, const uint8_t* flips,
                                     const int* jitter_order, const float* jitter_factors, const float* mean3, const float* std3, float* out,
                                     void* workspace, size_t workspace_bytes, sd_stream_t stream);
/* ... with the affine warp: affine and fill3 are required, the jitter is optional.  workspace: up to image B. */
size_t sd_preprocess_affine_workspace_bytes(int B, int Hin, int Win, int Hout, int Wout);
int sd_preprocess_images_affine(const uint8_t* images, int B, int Hin, int Win, int Hout, int Wout, const int* h_bounds, const int* h_kk,
                                int h_ksize, const int* v_bounds, const int* v_kk, int v_ksize, const uint8_t* flips, const int* jitter_order,
                                const float* jitter_factors, const double* affine, const uint8_t fill3[3], const float* mean3,
                                const float* std3, float* out, void* workspace, size_t workspace_bytes, sd_stream_t stream);
int sd_preprocess_images_list_affine(const uint8_t* const* images, int B, int Hin, int Win, int Hout, int Wout, const int* h_bounds,
                                     const int* h_kk, int h_ksize, const int* v_bounds, const int* v_kk, int v_ksize, const uint8_t* flips,
                                     const int* jitter_order, const float* jitter_factors, const double* affine, const uint8_t fill3[3],
                                     const float* mean3, const float* std3, float* out, void* workspace, size_t workspace_bytes,
                                     sd_stream_t stream);
/* ... with the mosaic: both mosaic tables and fill3 are required, the warp and the jitter are optional.  workspace: up to image B. */
size_t sd_preprocess_mosaic_workspace_bytes(int B, int Hin, int Win, int Hout, int Wout);
int sd_preprocess_images_mosaic(const uint8_t* images, int B, int Hin, int Win, int Hout, int Wout, const int* h_bounds, const int* h_kk,
                                int h_ksize, const int* v_bounds, const int* v_kk, int v_ksize, const uint8_t* flips, const int* jitter_order,
                                const float* jitter_factors, const double* affine, const int* mosaic_geom, const double* mosaic_affine,
                                const uint8_t fill3[3], const float* mean3, const float* std3, float* out, void* workspace,
                                size_t workspace_bytes, sd_stream_t stream);
int sd_preprocess_images_list_mosaic(const uint8_t* const* images, int B, int Hin, int Win, int Hout, int Wout, const int* h_bounds,
                                     const int* h_kk, int h_ksize, const int* v_bounds, const int* v_kk, int v_ksize, const uint8_t* flips,
                                     const int* jitter_order, const float* jitter_factors, const double* affine, const int* mosaic_geom,
                                     const double* mosaic_affine, const uint8_t fill3[3], const float* mean3, const float* std3, float* out,
                                     void* workspace, size_t workspace_bytes, sd_stream_t stream);
/* SD_GEOM_WINDOW with (Hg, Wg) = (Hc, Wc), g0 = max_rows, g1 = max_cols; every stage optional.  workspace: up to image B. */
size_t sd_preprocess_window_workspace_bytes(int B, int max_rows, int Hout, int Wout);
int sd_preprocess_images_window(const uint8_t* images, int B, int Hin, int Win, int Hc, int Wc, int Hout, int Wout, const int* h_bounds,
                                const int* h_kk, int h_ksize, const int* v_bounds, const int* v_kk, int v_ksize, const int* window, int max_rows,
                                int max_cols, const uint8_t* flips, const int* jitter_order, const float* jitter_factors, const double* affine,
                                const int* mosaic_geom, const double* mosaic_affine, const uint8_t fill3[3], const float* mean3, const float* std3,
                                float* out, void* workspace, size_t workspace_bytes, sd_stream_t stream);
int sd_preprocess_images_list_window(const uint8_t* const* images, int B, int Hin, int Win, int Hc, int Wc, int Hout, int Wout, const int* h_bounds,
                                     const int* h_kk, int h_ksize, const int* v_bounds, const int* v_kk, int v_ksize, const int* window,
                                     int max_rows, int max_cols, const uint8_t* flips, const int* jitter_order, const float* jitter_factors,
                                     const double* affine, const int* mosaic_geom, const double* mosaic_affine, const uint8_t fill3[3],
                                     const float* mean3, const float* std3, float* out, void* workspace, size_t workspace_bytes,
                                     sd_stream_t stream);
/* SD_GEOM_LETTERBOX with (Hg, Wg) = (Hi, Wi), g0 = y0, g1 = x0; every stage optional.  workspace: up to image B. */
size_t sd_preprocess_letterbox_workspace_bytes(int B, int Hin, int Wi, int Hout, int Wout);
int sd_preprocess_images_letterbox(const uint8_t* images, int B, int Hin, int Win, int Hi, int Wi, int Hout, int Wout, int y0, int x0,
                                   const int* h_bounds, const int* h_kk, int h_ksize, const int* v_bounds, const int* v_kk, int v_ksize,
                                   const uint8_t* flips, const int* jitter_order, const float* jitter_factors, const double* affine,
                                   const int* mosaic_geom, const double* mosaic_affine, const uint8_t fill3[3], const float* mean3,
                                   const float* std3, float* out, void* workspace, size_t workspace_bytes, sd_stream_t stream);
int sd_preprocess_images_list_letterbox(const uint8_t* const* images, int B, int Hin, int Win, int Hi, int Wi, int Hout, int Wout, int y0, int x0,
                                        const int* h_bounds, const int* h_kk, int h_ksize, const int* v_bounds, const int* v_kk, int v_ksize,
                                        const uint8_t* flips, const int* jitter_order, const float* jitter_factors, const double* affine,
                                        const int* mosaic_geom, const double* mosaic_affine, const uint8_t fill3[3], const float* mean3,
                                        const float* std3, float* out, void* workspace, size_t workspace_bytes, sd_stream_t stream);
/* Any geometry (geometry, Hg, Wg, g0, g1, window as in the descriptor), every stage optional, + blur.  workspace: up to image B. */
size_t sd_preprocess_blur_workspace_bytes(int geometry, int B, int Hin, int Win, int Wg, int Hout, int Wout, int g0);
int sd_preprocess_images_blur(const uint8_t* images, int geometry, int B, int Hin, int Win, int Hg, int Wg, int Hout, int Wout, int g0, int g1,
                              const int* h_bounds, const int* h_kk, int h_ksize, const int* v_bounds, const int* v_kk, int v_ksize,
                              const int* window, const uint8_t* flips, const int* jitter_order, const float* jitter_factors,
                              const double* affine, const int* mosaic_geom, const double* mosaic_affine, const int* blur,
                              const uint8_t fill3[3], const float* mean3, const float* std3, float* out, void* workspace,
                              size_t workspace_bytes, sd_stream_t stream);
int sd_preprocess_images_list_blur(const uint8_t* const* images, int geometry, int B, int Hin, int Win, int Hg, int Wg, int Hout, int Wout,
                                   int g0, int g1, const int* h_bounds, const int* h_kk, int h_ksize, const int* v_bounds, const int* v_kk,
                                   int v_ksize, const int* window, const uint8_t* flips, const int* jitter_order, const float* jitter_factors,
                                   const double* affine, const int* mosaic_geom, const double* mosaic_affine, const int* blur,
                                   const uint8_t fill3[3], const float* mean3, const float* std3, float* out, void* workspace,
                                   size_t workspace_bytes, sd_stream_t stream);
/* ... + persp after affine.  workspace: sd_preprocess_blur_workspace_bytes(). */
int sd_preprocess_images_persp(const uint8_t* images, int geometry, int B, int Hin, int Win, int Hg, int Wg, int Hout, int Wout, int g0, int g1,
                               const int* h_bounds, const int* h_kk, int h_ksize, const int* v_bounds, const int* v_kk, int v_ksize,
                               const int* window, const uint8_t* flips, const int* jitter_order, const float* jitter_factors,
                               const double* affine, const double* persp, const int* mosaic_geom, const double* mosaic_affine, const int* blur,
                               const uint8_t fill3[3], const float* mean3, const float* std3, float* out, void* workspace,
                               size_t workspace_bytes, sd_stream_t stream);
int sd_preprocess_images_list_persp(const uint8_t* const* images, int geometry, int B, int Hin, int Win, int Hg, int Wg, int Hout, int Wout,
                                    int g0, int g1, const int* h_bounds, const int* h_kk, int h_ksize, const int* v_bounds, const int* v_kk,
                                    int v_ksize, const int* window, const uint8_t* flips, const int* jitter_order, const float* jitter_factors,
                                    const double* affine, const double* persp, const int* mosaic_geom, const double* mosaic_affine,
                                    const int* blur, const uint8_t fill3[3], const float* mean3, const float* std3, float* out, void* workspace,
                                    size_t workspace_bytes, sd_stream_t stream);
/* ... + jpeg after blur.  workspace: the blur forms' + the decoded planes. */
size_t sd_preprocess_jpeg_workspace_bytes(int geometry, int B, int Hin, int Win, int Wg, int Hout, int Wout, int g0);
int sd_preprocess_images_jpeg(const uint8_t* images, int geometry, int B, int Hin, int Win, int Hg, int Wg, int Hout, int Wout, int g0, int g1,
                              const int* h_bounds, const int* h_kk, int h_ksize, const int* v_bounds, const int* v_kk, int v_ksize,
                              const int* window, const uint8_t* flips, const int* jitter_order, const float* jitter_factors,
                              const double* affine, const double* persp, const int* mosaic_geom, const double* mosaic_affine, const int* blur,
                              const int* jpeg, const uint8_t fill3[3], const float* mean3, const float* std3, float* out, void* workspace,
                              size_t workspace_bytes, sd_stream_t stream);
int sd_preprocess_images_list_jpeg(const uint8_t* const* images, int geometry, int B, int Hin, int Win, int Hg, int Wg, int Hout, int Wout,
                                   int g0, int g1, const int* h_bounds, const int* h_kk, int h_ksize, const int* v_bounds, const int* v_kk,
                                   int v_ksize, const int* window, const uint8_t* flips, const int* jitter_order, const float* jitter_factors,
                                   const double* affine, const double* persp, const int* mosaic_geom, const double* mosaic_affine,
                                   const int* blur, const int* jpeg, const uint8_t fill3[3], const float* mean3, const float* std3, float* out,
                                   void* workspace, size_t workspace_bytes, sd_stream_t stream);
/* ... + tone after jpeg.  workspace: the JPEG forms' + sd_tone_workspace_bytes(). */
size_t sd_preprocess_tone_workspace_bytes(int geometry, int B, int Hin, int Win, int Wg, int Hout, int Wout, int g0);
int sd_preprocess_images_tone(const uint8_t* images, int geometry, int B, int Hin, int Win, int Hg, int Wg, int Hout, int Wout, int g0, int g1,
                              const int* h_bounds, const int* h_kk, int h_ksize, const int* v_bounds, const int* v_kk, int v_ksize,
                              const int* window, const uint8_t* flips, const int* jitter_order, const float* jitter_factors,
                              const double* affine, const double* persp, const int* mosaic_geom, const double* mosaic_affine, const int* blur,
                              const int* jpeg, const int* tone, const uint8_t fill3[3], const float* mean3, const float* std3, float* out,
                              void* workspace, size_t workspace_bytes, sd_stream_t stream);
int sd_preprocess_images_list_tone(const uint8_t* const* images, int geometry, int B, int Hin, int Win, int Hg, int Wg, int Hout, int Wout,
                                   int g0, int g1, const int* h_bounds, const int* h_kk, int h_ksize, const int* v_bounds, const int* v_kk,
                                   int v_ksize, const int* window, const uint8_t* flips, const int* jitter_order, const float* jitter_factors,
                                   const double* affine, const double* persp, const int* mosaic_geom, const double* mosaic_affine,
                                   const int* blur, const int* jpeg, const int* tone, const uint8_t fill3[3], const float* mean3,
                                   const float* std3, float* out, void* workspace, size_t workspace_bytes, sd_stream_t stream);
/* ... + noise after tone (it runs between the blur and the JPEG round trip).  workspace: the tone forms' (the stage needs none). */
size_t sd_preprocess_noise_workspace_bytes(int geometry, int B, int Hin, int Win, int Wg, int Hout, int Wout, int g0);
int sd_preprocess_images_noise(const uint8_t* images, int geometry, int B, int Hin, int Win, int Hg, int Wg, int Hout, int Wout, int g0, int g1,
                               const int* h_bounds, const int* h_kk, int h_ksize, const int* v_bounds, const int* v_kk, int v_ksize,
                               const int* window, const uint8_t* flips, const int* jitter_order, const float* jitter_factors,
                               const double* affine, const double* persp, const int* mosaic_geom, const double* mosaic_affine, const int* blur,
                               const int* jpeg, const int* tone, const int* noise, const uint8_t fill3[3], const float* mean3, const float* std3,
                               float* out, void* workspace, size_t workspace_bytes, sd_stream_t stream);
int sd_preprocess_images_list_noise(const uint8_t* const* images, int geometry, int B, int Hin, int Win, int Hg, int Wg, int Hout, int Wout,
                                    int g0, int g1, const int* h_bounds, const int* h_kk, int h_ksize, const int* v_bounds, const int* v_kk,
                                    int v_ksize, const int* window, const uint8_t* flips, const int* jitter_order, const float* jitter_factors,
                                    const double* affine, const double* persp, const int* mosaic_geom, const double* mosaic_affine,
                                    const int* blur, const int* jpeg, const int* tone, const int* noise, const uint8_t fill3[3],
                                    const float* mean3, const float* std3, float* out, void* workspace, size_t workspace_bytes,
                                    sd_stream_t stream);

/* Gaussian blur of 8-bit images (training augmentation, `train --aug_blur`): image b becomes Image.filter(ImageFilter.GaussianBlur(r_b))
 * byte for byte -- Pillow's three box-blur passes along the rows, then three along the columns, each rounded to bytes.  blur (B, 3) int32
 * on the DEVICE = R, ww, fw per image, the whole box radius and the two 24-bit weights of one pass
 *     out[x] = (ww * sum_{i = -R .. R} in[c(x + i)] + fw * (in[c(x - R - 1)] + in[c(x + R + 1)]) + 2^23) >> 24,  c = clamp to the line,
 * computed on the host from r (data/augment.py blur_box_params; float32 arithmetic).  A row with R == 0 and fw == 0 (r = 0) copies its
 * image.  The table cannot be checked without a sync, so the kernels clamp R to [0, SD_BLUR_MAX_RADIUS]: any table is memory-safe (the
 * weights of a row that blurs are below 2^24 and enter as 24-bit factors; what a row outside the definition computes is unspecified).
 * SD_BLUR_MAX_RADIUS is the box radius of r = 8, the largest `--aug_blur` (sigma^2 = 64 / 3, l = floor((sqrt(257) - 1) / 2) = 7, box
 * radius 7.47).  in and out are (B, H, W, 3) uint8 and must not overlap (in place: SD_ERR_INVALID); workspace: sd_blur_workspace_bytes()
 * bytes (the image between the two directions). */
#define SD_BLUR_MAX_RADIUS 7
size_t sd_blur_workspace_bytes(int B, int H, int W);
int sd_blur_u8(const uint8_t* in, uint8_t* out, int B, int H, int W, const int* blur, void* workspace, size_t workspace_bytes,
               sd_stream_t stream);

/* Random perspective of 8-bit images (training augmentation, `train --aug_perspective`): image b becomes
 * Image.transform((W, H), PERSPECTIVE, coeffs_b, BILINEAR, fillcolor=fill3) byte for byte.  coeffs (B, 8) fp64 on the DEVICE = a0 .. a7:
 * with xc = x + 0.5, yc = y + 0.5 the output pixel (x, y) samples the source position
 *     den = a6 xc + a7 yc + 1,  xin = (a0 xc + a1 yc + a2) / den,  yin = (a3 xc + a4 yc + a5) / den
 * (every product and sum rounded on its own, left to right; two correctly rounded fp64 divisions) exactly as the affine warp samples its
 * position: the inside test, the -0.5 shift, floor, clamped taps, the double lerp, truncation to a byte.  A position that is infinite or
 * NaN is outside and becomes fill; where den is negative a position inside the source is sampled, as in Pillow.  A row with a6 = a7 = 0
 * gives the bytes of the affine warp with the same six coefficients.  Nothing in a row is validated: index clamps bound every address for
 * any table.  in and out are (B, H, W, 3) uint8 and must not overlap; fill3 is a HOST pointer.  B <= 65535. */
int sd_perspective_u8(const uint8_t* in, uint8_t* out, int B, int H, int W, const double* coeffs, const uint8_t fill3[3], sd_stream_t stream);

/* JPEG compression of 8-bit images (training augmentation, `train --aug_jpeg`): image b becomes what Pillow's
 * Image.save(buf, "JPEG", qtables=[ql_b, qc_b], subsampling=2) followed by Image.open(buf) gives, byte for byte: libjpeg's RGB -> YCbCr,
 * h2v2 chroma downsampling, accurate-integer forward DCT, quantiser, dequantiser, accurate-integer inverse DCT, h2v2 "fancy" chroma
 * upsampling and YCbCr -> RGB, all in 32-bit integers (the entropy coder is lossless and is left out; tests/jpeg_ref.py states every
 * formula).  table (B, 129) int32 on the DEVICE: a row is [on, ql[64], qc[64]], the luminance and chrominance quantisation tables in
 * natural (row-major) order, e.g. libjpeg's standard tables at a quality (data/augment.py jpeg_quant_tables).  A row with on == 0 copies
 * its image.  Entries outside [1, 255] are clamped into that range; nothing in a row decides an address, so any table is memory-safe.
 * in and out are (B, H, W, 3) uint8 with H and W multiples of 16 (whole MCUs; SD_ERR_INVALID otherwise); out may be in (in place), any
 * other overlap is SD_ERR_INVALID.  workspace: sd_jpeg_workspace_bytes() bytes, 16-byte aligned -- the decoded Y plane at full size and
 * the decoded Cb and Cr planes at half size.  Two launches.  B <= 65535. */
size_t sd_jpeg_workspace_bytes(int B, int H, int W);
int sd_jpeg_u8(const uint8_t* in, uint8_t* out, int B, int H, int W, const int* table, void* workspace, size_t workspace_bytes,
               sd_stream_t stream);

/* Histogram tone curves of 8-bit images (training augmentation, `train --aug_equalize / --aug_autocontrast`): image b becomes what Pillow's
 * ImageOps.equalize(img) (mode 2) or ImageOps.autocontrast(img, cutoff) (mode 1) gives, byte for byte: per channel a 256-bin histogram of
 * the image's own pixels, a 256-entry table made from it, a look-up (tests/tone_ref.py states both tables; equalize is 32-bit unsigned
 * integer arithmetic, autocontrast one IEEE double expression whose product and sum are rounded separately).  table (B, 4) int32 on the
 * DEVICE: a row is [mode, cut_lo, cut_hi, 0]; cut_lo / cut_hi are the numbers of darkest / brightest pixels autocontrast ignores, Pillow's
 * int(H * W * cutoff // 100) (data/augment.py tone_rows).  Mode 0 and every mode other than 1 and 2 copies its image.  The cuts are
 * clamped to [0, H * W]; nothing in a row decides an address, so any table is memory-safe.  in and out are (B, H, W, 3) uint8, any
 * H, W >= 1 with H * W < 2^31 and any byte alignment; out may be in (in place), any other overlap is SD_ERR_INVALID.  workspace:
 * sd_tone_workspace_bytes() bytes, 16-byte aligned -- the (B, 3, 256) uint32 histograms (the tables are made in LDS by the look-up
 * launch).  One memset and two launches; a histogram block covers SD_TONE_STRIP_PIXELS pixels of one image.  B <= 65535. */
#define SD_TONE_STRIP_PIXELS 16384
size_t sd_tone_workspace_bytes(int B);
int sd_tone_u8(const uint8_t* in, uint8_t* out, int B, int H, int W, const int* table, void* workspace, size_t workspace_bytes,
               sd_stream_t stream);

/* Sensor noise on 8-bit images (training augmentation, `train --aug_noise / --aug_noise_shot`): read noise plus signal-dependent shot noise,
 * the heteroscedastic-Gaussian sensor model per channel and pixel in the 8-bit domain (no gamma is modelled), all integer and bit-exact:
 * with o the byte's offset inside ITS image, word = Philox4x32-10(counter (o >> 2, 0, 0, 0), key (k0, k1))[o & 3]; z = the unit normal in
 * Q10 from the word's top 12 bits through a 2048-entry inverse-CDF half table (the other 20 bits are not used); sigma(v) = isqrt(a' + b' v)
 * in Q8 with a' = min(a, 2^26), b' = min(b, 2^17); out = clamp(v + ((z sigma(v) + 2^17) >> 18), 0, 255) (tests/noise_ref.py restates it).
 * table (B, 4) int32 on the DEVICE: a row is [k0, k1, a, b], a = the read-noise variance and b = the shot gain per level, both in Q16
 * levels^2 and read as uint32 (data/augment.py noise_rows); the clamps are part of the definition and nothing in a row decides an address,
 * so any table is memory-safe; a row with a' = b' = 0 leaves its image as it is.  The bytes depend on the image's content and its row only,
 * not on the launch shape, the position in the batch or the base address.  in and out are (B, H, W, 3) uint8, any H, W >= 1 with
 * H * W < 2^31 and any byte alignment; out may be in (in place), any other overlap is SD_ERR_INVALID.  One launch, no workspace.
 * B <= 65535.  sd_noise_normal_table (host only) copies the half table H[j] = round(1024 Phi^-1((2048 + j + 0.5) / 4096)). */
int sd_noise_normal_table(uint16_t out[2048]);
int sd_noise_u8(const uint8_t* in, uint8_t* out, int B, int H, int W, const int* table, sd_stream_t stream);

/* ---- loss: src/sdnet/model/loss.py:17-64,91-117------------------------------------------- */

#define SD_HM_MSE   0
#define SD_HM_FOCAL 1

typedef struct sd_loss_desc {
    /* head output, network.py:77-84 (strided channel-slice views allowed) */
    const float* anchor_hm;  int64_t a_sb, a_sc;      /* (B,M,h,w) logits */
    const float* part_hm;    int64_t p_sb, p_sc;      /* (B,N,h,w) logits */
    const float* offsets;    int64_t o_sb, o_sc;      /* (B,2,h,w) */
    const float* embeddings; int64_t e_sb, e_sc;      /* (B,2,h,w) */
    /* collated Encode output, dataset.py:58-87 */
    const float* t_anchor_hm; int64_t ta_sb, ta_sc;   /* (B,M,h,w) */
    const float* t_part_hm;   int64_t tp_sb, tp_sc;   /* (B,N,h,w) */
    const int64_t* anchor_inds;   /* (B,K) */
    const int64_t* part_inds;     /* (B,P) */
    const float* anchor_offsets;  /* (B,K,2) */
    const float* part_offsets;    /* (B,P,2) */
    const float* t_embeddings;    /* (B,P,2) */
    const uint8_t* anchor_mask;   /* (B,K) bool */
    const uint8_t* part_mask;     /* (B,P) bool */
    int B, M, N, h, w, K, P;
    int hm_loss_fn;               /* SD_HM_MSE | SD_HM_FOCAL (args.py:96-102) */
    float hm_weight, offset_weight, embedding_weight;   /* args.py:118-132 */
} sd_loss_desc;

/* Loss.forward (loss.py:17-50).  out[0..3] = total, hm, offset, embedding (weighted, as
 * LossStats loss.py:120-165); out[4..7] = num_pos(anchor), num_pos(part), #valid anchors,
 * #valid parts (kept on device for the backward; no host branch, cf. loss.py:59-61,110). */
size_t sd_loss_workspace_bytes(int B, int M, int N, int h, int w);
int sd_loss_fwd(const sd_loss_desc* d, float* out8, void* workspace, size_t workspace_bytes, sd_stream_t stream);

/* Loss.forward of every image of the batch on its own (validation: per-image losses, then the mean over
 * images, trainer.py:160-168).  out: (B,8) device floats, row b = sd_loss_fwd's out8 of image b alone and
 * bit-identical to a separate B = 1 sd_loss_fwd call.  Same descriptor and workspace
 * (sd_loss_workspace_bytes) as sd_loss_fwd; two launches for the whole batch. */
int sd_loss_fwd_per_image(const sd_loss_desc* d, float* out, void* workspace, size_t workspace_bytes, sd_stream_t stream);

/* d total / d head for all M+N+4 channels.  grad_out: device scalar (upstream gradient).
 * dhead: (B,M+N+4,h,w) contiguous, fully overwritten. */
int sd_loss_bwd(const sd_loss_desc* d, const float* out8, const float* grad_out, float* dhead, sd_stream_t stream);


/* ---- network: src/sdnet/model/network.py:6-87 (+ torchvision resnet34 BasicBlocks) --------
 * Activations are NHWC fp32 (torch channels_last), weights [Cout][R][S][Cin] (torch
 * channels_last OIHW).  These entry points replace the torch.nn.Conv2d / BatchNorm2d / ReLU /
 * MaxPool2d / Upsample modules the reference composes, and torch.optim.Adam
 * (src/sdnet/model/trainer.py:53,124). */

typedef struct sd_conv_desc {
    int B, Hi, Wi, Cin, Ho, Wo, Cout, R, S, stride, pad;
} sd_conv_desc;

/* y = [relu]( conv(x, w) * scale[co] + shift[co] [+ residual] ), fp32 MFMA implicit GEMM.
 * scale/shift/residual nullable.  res_up2: residual is the (Ho/2, Wo/2) map, nearest-upsampled x2
 * (Fpn.forward, network.py:18-19).  Needs Cin % 32 == 0, Cout % 64 == 0.  When the tile grid cannot fill
 * the chip (small batch) and a workspace is supplied, K is split over blocks and a second pass applies the epilogue. */
size_t sd_conv2d_fwd_workspace_bytes(const sd_conv_desc* d);   /* > 0 only when split-K pays (small batch) */
int sd_conv2d_fwd(const float* x_nhwc, const float* w_krsc, float* y_nhwc, const sd_conv_desc* d,
                  const float* scale, const float* shift, const float* residual, int res_up2, int relu,
                  void* workspace, size_t workspace_bytes, sd_stream_t stream);
/* stem: 7x7/2 conv 3 -> 64 reading the NCHW image directly (network.py:43; resnet.conv1). */
size_t sd_conv2d_stem_fwd_workspace_bytes(const sd_conv_desc* d);
int sd_conv2d_stem_fwd(const float* x_nchw, const float* w_krsc, void* y_nhwc, const sd_conv_desc* d,
                       const float* scale, const float* shift, int relu, int out_bf16, void* workspace,
                       size_t workspace_bytes, sd_stream_t stream);

/* Small-batch inference forward (the batch-1 evaluate loop, src/sdnet/cli/evaluate.py:34-45 -> network.py:59-84): same
 * arithmetic and epilogue as sd_conv2d_fwd / sd_conv2d_fwd_bf16 (bf16 != 0: x, w, y, residual are bf16, accumulation and epilogue
 * fp32) on 64-pixel x 64-channel tiles with the reduction split over blocks so that tiles x slices is about one block per CU; the
 * partial tiles are combined INSIDE the launch by the block that arrives last for a tile (summed in slice order: results do not
 * depend on the arrival order), so a conv is ONE launch.  sd_conv2d_fwd_sb_supported(): 1 for the geometries it is meant for
 * (the 128-row tile grid of sd_conv2d_fwd would not fill the chip twice: batches up to ~16 at 512x512); any R == S conv with Cin % 32 (bf16: 64) == 0, Cout % 64 == 0
 * is computed correctly.  `workspace`: sd_conv2d_fwd_sb_workspace_bytes() of scratch (partial tiles; no initialisation).
 * `state`: sd_conv2d_fwd_sb_state_bytes() bytes owned by the caller, used by nothing else that may run concurrently, ZERO before
 * the first call; every call leaves it zero again (back-to-back launches and hipGraph replays need no memset).  After a failed
 * or aborted launch re-zero it.  Both may be null / 0 when sd_conv2d_fwd_sb_workspace_bytes() is 0 (no split). */
int    sd_conv2d_fwd_sb_supported(const sd_conv_desc* d, int bf16);
size_t sd_conv2d_fwd_sb_workspace_bytes(const sd_conv_desc* d, int bf16);
size_t sd_conv2d_fwd_sb_state_bytes(const sd_conv_desc* d, int bf16);
int sd_conv2d_fwd_sb(const void* x_nhwc, const void* w_krsc, void* y_nhwc, const sd_conv_desc* d, const float* scale, const float* shift,
                     const void* residual, int res_up2, int relu, int bf16, void* workspace, size_t workspace_bytes, void* state,
                     size_t state_bytes, sd_stream_t stream);

/* The stem conv (7x7 / 2 / 3, NCHW image -> NHWC fp32) with the batch statistics of its output from the same launch
 * (as sd_conv2d_fwd_bn_stats; one pass over the 16.8 MB/img stem output less). */
size_t sd_conv2d_stem_fwd_bn_stats_workspace_bytes(const sd_conv_desc* d);
int sd_conv2d_stem_fwd_bn_stats(const float* x_nchw, const float* w, float* y, const sd_conv_desc* d, float eps, float momentum,
                                float* running_mean, float* running_var, float* mean, float* invstd, void* workspace,
                                size_t workspace_bytes, sd_stream_t stream);

/* Training forward of a conv that feeds a BatchNorm2d: y = conv(x, w) and, from the accumulators of the same launch, the batch
 * statistics of y (mean, invstd = 1/sqrt(biased var + eps), running-stat update as sd_bn_train_stats) -- one pass over y less
 * than sd_conv2d_fwd + sd_bn_train_stats.  Partial sums per (tile, wave row) go through `workspace` and are finished in double
 * precision in a fixed order (deterministic).  Falls back to the two-pass form when the forward splits K (tiny batches). */
size_t sd_conv2d_fwd_bn_stats_workspace_bytes(const sd_conv_desc* d);
int sd_conv2d_fwd_bn_stats(const float* x, const float* w, float* y, const sd_conv_desc* d, float eps, float momentum,
                           float* running_mean, float* running_var, float* mean, float* invstd, void* workspace,
                           size_t workspace_bytes, sd_stream_t stream);
/* second half of sd_bn_train_stats on caller-provided partial sums [rows][2][C] (sum, sum of squares per channel); `scratch`
 * (nullable) = sd_bn_finalize_scratch_rows(rows) * 2 * C floats for the coalesced first folding level used with many rows */
int sd_bn_finalize_scratch_rows(int rows);
int sd_bn_finalize_stats(const float* partial, int rows, int64_t M, int C, float eps, float momentum, float* running_mean,
                         float* running_var, float* mean, float* invstd, float* scratch, sd_stream_t stream);

/* Data-gradient of a conv whose INPUT was the output of a BatchNorm2d (+ReLU): dx = dgrad(dy) [+ residual] as sd_conv2d_dgrad,
 * and from the values of the same epilogue the reduction of that BatchNorm's backward (sum g, sum g * xhat per channel with
 * g = dx * relu mask, xhat = (bn_x - mean) * invstd; relu as in sd_bn_bwd) -- one pass over dx and bn_x less than
 * sd_conv2d_dgrad + sd_bn_bwd.  Writes dgamma / dbeta (+= when accumulate) and means_out = [mean(g) (C), mean(g xhat) (C)],
 * C = Cin; finish with sd_bn_bwd_apply(dy = dx, x = bn_x, ...).  Deterministic (partials per tile, fixed-order finish). */
size_t sd_conv2d_dgrad_bn_reduce_workspace_bytes(const sd_conv_desc* d);
int sd_conv2d_dgrad_bn_reduce(const float* dy, const float* w_t, float* dx, const sd_conv_desc* d, const float* residual,
                              const float* bn_x, const float* bn_y, int relu, const float* mean, const float* invstd,
                              const float* gamma, const float* beta, float* dgamma, float* dbeta, int accumulate,
                              float* means_out, void* workspace, size_t workspace_bytes, sd_stream_t stream);
/* the two halves of sd_bn_bwd after its reduction pass */
int sd_bn_bwd_finalize(const float* partial, int rows, int64_t M, int C, float* dgamma, float* dbeta, int accumulate,
                       float* means_out, float* scratch, sd_stream_t stream);
int sd_bn_bwd_apply(const float* dy, const float* x, const float* y, int relu, int64_t M, int C, const float* mean,
                    const float* invstd, const float* gamma, const float* beta, const float* means, float* dx, float* g_out,
                    sd_stream_t stream);

/* Kernel-selection thresholds (tuning / test switches; they never change results beyond fp32 summation order).  THREAD-LOCAL: a value
 * applies to the calls made by the host thread that set it and every thread starts from the defaults -- two engines driven from two
 * threads of one process (training + evaluation) cannot change each other's kernel choice; the library keeps no process-global
 * mutable state.  sd_conv2d_kernel_name() reports the choice the CALLING thread would get.  "conv_patch_min_tiles": smallest tile grid for which the 3x3 stride-1 convs take the
 * patch-staging kernel (default 512 = two resident blocks per CU; 1 = always, for tests; 1 << 30 = never);
 * "conv_patch_bn64": 1 = also for layers with 64 output channels (default 0: slower inside the training step);
 * "conv_pp_min_tiles": smallest grid of 512-pixel x 128-channel tiles for which the bf16 3x3 stride-1 convs take the two-group
 * kernel k_conv3x3_bf16_pp (default 200; 1 = always, for tests; 1 << 30 = never); "conv_patch_narrow": layers whose 128-channel patch
 * tiles do not fill the chip fall back to 64-channel patch tiles (0 never, 1 fp32 only, 2 = default: fp32 and bf16); "conv_pp_strips": 0 = maps of 128 pixels and wider are
 * not cut into 64-pixel column strips for that kernel (default 1; A/B measurements); "conv_fwd_split_k": 0 = the forward convs never
 * split K over blocks (default 1: small grids do), so that tests can put small problems on the single-pass kernels;
 * "conv_rows64_min_units": smallest number of (image, 128-pixel strip, row range) units for which the bf16 64 -> 64 channel 3x3 convs take
 * the row-stream kernel k_conv3x3_c64_rows_bf16 (default 192, and at least 16 rows per unit; 1 = always, for tests; 1 << 30 = never);
 * "conv_rows_f32_min_units": the same for the fp32 row-stream kernel k_conv3x3_c64_rows_f32 (units = image x 64-pixel strip x row range).
 * "conv1x1_stream_min_pixels": smallest number of output pixels for which a bf16 1x1 / stride 1 conv onto 128 channels (Cin 64 or 128, no
 *   scale, no statistics: the FPN laterals and the 128 -> 128 1x1 data-gradient) takes the stream kernel k_conv1x1_stream_bf16 (default
 *   65536; 32 = always, for tests; 1 << 30 = never).
 * "wgrad_f32_ring": form of the fp32 weight gradient of the 3x3 / stride 1 layers with maps a multiple of 32 pixels wide: 2 (default) =
 *   k_wgrad3x3_ring2 (row ring: one new patch row per chunk; two groups of four waves per 512-thread block share a tile and store ONE partial),
 *   1 = k_wgrad3x3_ring (one group per block), 0 = the first form k_wgrad3x3<32> (A/B, tests).
 * "wgrad_bf16_ring": form of the bf16 weight gradient of the 3x3 / stride 1 layers with maps a multiple of 32 pixels wide: 5 (default) =
 *   k_wgrad3x3_bf16_ring2 (row ring, two groups of four waves half a chunk apart in one 512-thread block), 2 .. 4 = k_wgrad3x3_bf16_ring with
 *   that prefetch distance, 0 = the first form k_wgrad3x3_bf16<32> (A/B, tests).
 * "stem_fwd_blocks": persistent blocks of the fp32 training stem forward (default 512 = two per CU; 256 = one per CU, the setting the
 *   in-kernel phase trace of tools/stem_trace_f32.py compares against). */
int sd_set_option(const char* name, int value);

/* Name of the device kernel the launchers pick for this geometry (pass 0 = sd_conv2d_fwd, 1 = sd_conv2d_dgrad,
 * 2 = sd_conv2d_wgrad; 16 = sd_conv2d_fwd_bf16, 17 = sd_conv2d_dgrad_bf16), as rocprofv3 prints it without the sd:: namespace -- lets a profiler label its event timings
 * with the same names as the kernel trace.  Passes 0 / 1 / 16 / 17 name the kernel of the dispatch plan (plan_conv in csrc/sd_conv.hip, the
 * same function the launchers run) of a launch WITHOUT epilogue operands: a launch with a scale, fused statistics or a half-size residual can
 * take another kernel (a 1x1 conv named k_conv1x1_stream_bf16 runs k_conv_igemm then).  Thread-local storage, valid until the next call on the thread. */
const char* sd_conv2d_kernel_name(const sd_conv_desc* d, int pass);

/* bf16 backbone (inference; BASELINE stress config "bf16 backbone + fp32 decode"): activations and weights bf16
 * NHWC / [Cout][R][S][Cin], v_mfma_f32_32x32x16_bf16 with fp32 accumulation and fp32 epilogue (folded BN, bias,
 * residual, ReLU), bf16 stores.  Needs Cin % 64 == 0. */
int sd_cast_f32_to_bf16(const float* x, void* y_bf16, int64_t n, sd_stream_t stream);
size_t sd_conv2d_fwd_bf16_workspace_bytes(const sd_conv_desc* d);
int sd_conv2d_fwd_bf16(const void* x_nhwc_bf16, const void* w_krsc_bf16, void* y_nhwc_bf16, const sd_conv_desc* d,
                       const float* scale, const float* shift, const void* residual_bf16, int res_up2, int relu,
                       void* workspace, size_t workspace_bytes, sd_stream_t stream);
int sd_maxpool3x3s2_fwd_bf16(const void* x_bf16, void* y_bf16, int B, int Hi, int Wi, int C, sd_stream_t stream);
/* network.py:59-63 `adpater` (conv1 7x7/s2 -> bn1 -> relu -> maxpool 3x3/s2) in ONE launch for the bf16 backbone: fp32 NCHW image, fp32
 * weights [64][7][7][3], folded BatchNorm scale / shift, pooled NHWC bf16 output [B][Ho/2][Wo/2][64] (d describes the conv: Ho, Wo even).
 * The full-resolution activation is never written.  Same values as sd_conv2d_stem_fwd(out_bf16 = 1) + sd_maxpool3x3s2_fwd_bf16 up to
 * the fp32 summation order of the conv (<= 1 bf16 ulp). */
int sd_stem_bn_relu_maxpool_fwd_bf16(const float* x_nchw, const float* w, const float* scale, const float* shift, void* y_bf16,
                                     const sd_conv_desc* d, sd_stream_t stream);

/* ---- mixed-precision training: the step the reference runs under `--amp` (src/sdnet/model/trainer.py:115-121: the forward and
 * the loss inside torch.autocast, backward in the dtypes the forward used, fp32 master weights updated by Adam).  Activations and
 * the weights handed to the convs are bf16, every accumulation (MFMA, BatchNorm statistics, gradients of parameters) is fp32.
 * BatchNorm statistics are those of the bf16-ROUNDED conv output (the tensor that is normalised, as under autocast). */
int sd_cast_bf16_to_f32(const void* x_bf16, float* y, int64_t n, sd_stream_t stream);
size_t sd_conv2d_fwd_bf16_bn_stats_workspace_bytes(const sd_conv_desc* d);
int sd_conv2d_fwd_bf16_bn_stats(const void* x_nhwc_bf16, const void* w_krsc_bf16, void* y_nhwc_bf16, const sd_conv_desc* d, float eps,
                                float momentum, float* running_mean, float* running_var, float* mean, float* invstd,
                                void* workspace, size_t workspace_bytes, sd_stream_t stream);
/* sd_conv2d_stem_fwd_bn_stats with the product on the bf16 MFMA (operands rounded on the way in; fp32 output and statistics). */
int sd_conv2d_stem_fwd_bn_stats_bf16mm(const float* x_nchw, const float* w, float* y, const sd_conv_desc* d, float eps, float momentum,
                                       float* running_mean, float* running_var, float* mean, float* invstd,
                                       void* workspace, size_t workspace_bytes, sd_stream_t stream);
/* ... and with a bf16 NHWC output (statistics of the rounded values): the mixed-precision step's stem; its tail reads that tensor through
 * sd_bn_relu_maxpool_fwd_bf16 / sd_maxpool_bn_relu_bwd_bf16 (fp32 arithmetic, bf16 conv output / pooled map / pooled gradient, fp32 dx). */
int sd_conv2d_stem_fwd_bn_stats_bf16(const float* x_nchw, const float* w, void* y_bf16, const sd_conv_desc* d, float eps, float momentum,
                                     float* running_mean, float* running_var, float* mean, float* invstd, void* workspace,
                                     size_t workspace_bytes, sd_stream_t stream);
int sd_bn_relu_maxpool_fwd_bf16(const void* x_bf16, int B, int Hi, int Wi, int C, const float* mean, const float* invstd, const float* gamma,
                                const float* beta, void* y_pool_bf16, uint8_t* idx, sd_stream_t stream);
int sd_maxpool_bn_relu_bwd_bf16(const void* dpool_bf16, const uint8_t* idx, const void* x_bf16, int B, int Hi, int Wi, int C, const float* mean,
                                const float* invstd, const float* gamma, const float* beta, float* dx, float* dgamma, float* dbeta, int accumulate,
                                void* workspace, size_t workspace_bytes, sd_stream_t stream);
/* ... and with the input gradient stored as bf16 (what autocast hands the stem conv's backward: trainer.py:116-121 runs conv1 in bf16):
 * half the bytes written here and read by sd_conv2d_stem_wgrad_bf16.  dgamma / dbeta as above (fp32 sums of the fp32 values). */
int sd_maxpool_bn_relu_bwd_bf16_dx16(const void* dpool_bf16, const uint8_t* idx, const void* x_bf16, int B, int Hi, int Wi, int C, const float* mean,
                                     const float* invstd, const float* gamma, const float* beta, void* dx_bf16, float* dgamma, float* dbeta,
                                     int accumulate, void* workspace, size_t workspace_bytes, sd_stream_t stream);
/* [Cout][taps][Cin] fp32 -> [Cin][taps][Cout] bf16 in one pass (the data-gradient's weights under --amp). */
int sd_conv2d_transpose_weights_bf16(const float* w, void* w_t_bf16, int Cout, int taps, int Cin, sd_stream_t stream);

/* Inference: the last FPN convolution (network.py:17-18: conv3x3 + folded BatchNorm + ReLU onto fpn_depth = 128 channels) with the network's
 * 1x1 head (network.py:22-29) applied to every output tile in the kernel's epilogue -- the FPN output tensor (268 MB in bf16 at bs = 64,
 * 512x512) is neither written nor read back, and the head launch disappears.  head_y = fp32 NCHW (B, head_co, Ho, Wo), the tensor
 * Network.forward slices into its four views (network.py:77-84).  `head_prepared` = sd_head_split_bf16_bytes() bytes written by
 * sd_head_split_bf16 from the fp32 head weights [head_co][128] and bias (hi / lo bf16 halves, zero padded to 32 rows: once per set of
 * weights).  sd_conv2d_fwd_bf16_head_supported = 1 where the convolution takes k_conv3x3_bf16_pp (bs = 64 at 512x512, bs = 16 at
 * 1024x1024, ...); elsewhere call sd_conv2d_fwd_bf16 + sd_head_fwd_bf16. */
int sd_conv2d_fwd_bf16_head_supported(const sd_conv_desc* d, int head_co);
size_t sd_head_split_bf16_bytes(void);
int sd_head_split_bf16(const float* head_w, const float* head_bias, int head_co, void* prepared, sd_stream_t stream);
int sd_conv2d_fwd_bf16_head(const void* x_bf16, const void* w_bf16, const sd_conv_desc* d, const float* scale, const float* shift, int relu,
                            const void* head_prepared, int head_co, float* head_y, sd_stream_t stream);
/* dx = dgrad(dy) [+ residual]: bf16 dy / transposed weights [Cin][R][S][Cout] / dx; res_mode 0 none, 1 bf16 tensor of dx's shape,
 * 2 bf16 half-size map added at the even pixels (the 1x1 / stride-2 downsample branch). */
int sd_conv2d_dgrad_bf16(const void* dy_bf16, const void* w_t_bf16, void* dx_bf16, const sd_conv_desc* d, const void* residual_bf16,
                         int res_mode, sd_stream_t stream);
/* dW (fp32, into the flat gradient buffer) from bf16 dy and bf16 x: 3x3 / stride 1 / pad 1 layers on the bf16 MFMA (transposed LDS
 * reads, all nine taps per block), the strided and 1x1 convs through the fp32 kernels on widened operands. */
size_t sd_conv2d_wgrad_bf16_workspace_bytes(const sd_conv_desc* d);
int sd_conv2d_wgrad_bf16(const void* dy_bf16, const void* x_nhwc_bf16, float* dw_krsc, const sd_conv_desc* d, int accumulate,
                         void* workspace, size_t workspace_bytes, sd_stream_t stream);
/* sd_bn_apply / sd_bn_bwd / sd_col_sum / sd_upsample2x_bwd on bf16 activations (parameters, statistics and parameter gradients fp32;
 * arithmetic in fp32, one rounding at the store). */
int sd_bn_apply_bf16(const void* x, void* y, int64_t M, int C, const float* mean, const float* invstd, const float* gamma,
                     const float* beta, const void* residual, int relu, uint8_t* relu_mask_out, sd_stream_t stream);
int sd_bn_bwd_bf16(const void* dy, const void* x, const void* y, int relu, int64_t M, int C, const float* mean, const float* invstd,
                   const float* gamma, const float* beta, void* dx, void* g_out, float* dgamma, float* dbeta, int accumulate,
                   void* workspace, size_t workspace_bytes, sd_stream_t stream);
int sd_bn_train_stats_bf16(const void* x, int64_t M, int C, float eps, float momentum, float* running_mean, float* running_var,
                           float* mean, float* invstd, void* workspace, size_t workspace_bytes, sd_stream_t stream);
int sd_col_sum_bf16(const void* x, int64_t M, int C, float* out, int accumulate, void* workspace, size_t workspace_bytes, sd_stream_t stream);
int sd_upsample2x_bwd_bf16(const void* dy, const void* add, void* dx, int B, int H, int W, int C, sd_stream_t stream);
int sd_head_fwd_bf16(const void* x_nhwc_bf16, const float* w, const float* bias, float* y_nchw, int B, int HW, int C,
                     int Co, sd_stream_t stream);
/* dX = conv_transpose(dY, W): same kernel with the inverted coordinate map; w_t = weights
 * re-laid as [Cin][R][S][Cout] by sd_conv2d_transpose_weights.  residual (nullable, same layout as
 * dX) is added (skip-connection gradient). */
int sd_conv2d_dgrad(const float* dy_nhwc, const float* w_t, float* dx_nhwc, const sd_conv_desc* d,
                    const float* residual, sd_stream_t stream);
/* The same with a residual that only exists on the even pixels: residual_half is (B, Hi/2, Wi/2, Cin) and is added to
 * dx[b, 2y, 2x, :] -- the data-gradient of a 1x1 / stride 2 "downsample" branch (network: BasicBlock.downsample) is zero on
 * three of four pixels, so it is computed as the stride-1 1x1 data-gradient on the small map and joined here instead of being
 * zero-filled to full size and read back. */
int sd_conv2d_dgrad_half_res(const float* dy, const float* w_t, float* dx, const sd_conv_desc* d, const float* residual_half,
                             sd_stream_t stream);
int sd_conv2d_transpose_weights(const float* w, float* w_t, int Cout, int taps, int Cin, sd_stream_t stream);
/* The same transpose for MANY convs in one launch (a training step re-lays every conv's weights once per backward).  table (device,
 * 8 ints per conv): {offset of w in w_base, offset of w_t in w_t_base (elements), Cout, taps, Cin, first block, ceil(Cin/32),
 * ceil(Cout/32)}; a conv owns ceil(Cin/32) * ceil(Cout/32) * taps consecutive blocks; out_bf16: w_t_base is bf16 (mixed precision). */
int sd_conv2d_transpose_weights_batched(const float* w_base, void* w_t_base, const int* table, int nconv, int total_blocks, int out_bf16,
                                        sd_stream_t stream);
/* dW[co][r][s][ci] (+)= sum_pixels dY * X, split over pixel ranges + deterministic reduce. */
size_t sd_conv2d_wgrad_workspace_bytes(const sd_conv_desc* d);
int sd_conv2d_wgrad(const float* dy_nhwc, const float* x_nhwc, float* dw_krsc, const sd_conv_desc* d,
                    int accumulate, void* workspace, size_t workspace_bytes, sd_stream_t stream);
/* stem weight gradient from the NCHW image: dW [64][7][7][3]. */
size_t sd_conv2d_stem_wgrad_workspace_bytes(const sd_conv_desc* d);
int sd_conv2d_stem_wgrad(const float* dy_nhwc, const float* x_nchw, float* dw_krsc, const sd_conv_desc* d,
                         int accumulate, void* workspace, size_t workspace_bytes, sd_stream_t stream);
/* ... with the product on the bf16 MFMA (mixed-precision training): dy and the image are rounded to bf16 on their way into the operands,
 * the sums and dw stay fp32.  Same workspace. */
int sd_conv2d_stem_wgrad_bf16mm(const float* dy, const float* x_nchw, float* dw, const sd_conv_desc* d, int accumulate, void* workspace,
                                size_t workspace_bytes, sd_stream_t stream);
/* ... from a bf16 dy [M][64] (16-byte aligned): the mixed-precision step's stem (row-ring kernel: a block walks down a 128-pixel column
 * strip and fetches two new image rows per tile; dy by LDS-DMA, transposed by ds_read_b64_tr_b16).  Same workspace, fp32 sums and dw. */
int sd_conv2d_stem_wgrad_bf16(const void* dy_bf16, const float* x_nchw, float* dw, const sd_conv_desc* d, int accumulate, void* workspace,
                              size_t workspace_bytes, sd_stream_t stream);

/* BatchNorm2d over [M][C] (M = B*H*W): training statistics (biased var for normalisation,
 * running stats with momentum and the unbiased var, torch semantics), apply (+residual, +ReLU),
 * eval-mode fold into (scale, shift), backward (dy masked by y > 0 when relu; g_out optionally
 * receives the masked gradient for the skip connection). */
size_t sd_col_reduce_workspace_bytes(int64_t M, int C);
int sd_bn_train_stats(const float* x, int64_t M, int C, float eps, float momentum, float* running_mean,
                      float* running_var, float* mean, float* invstd, void* workspace, size_t workspace_bytes,
                      sd_stream_t stream);
/* relu_mask_out (nullable): M*C/4 bytes, bit j of byte i = element 4i+j of the result is positive -- the ReLU mask the backward of a
 * residual layer needs, at 1/16 of the bytes of y (relu mode 3 of sd_bn_bwd / sd_bn_bwd_apply / sd_conv2d_dgrad_bn_reduce). */
int sd_bn_apply(const float* x, float* y, int64_t M, int C, const float* mean, const float* invstd,
                const float* gamma, const float* beta, const float* residual, int relu, uint8_t* relu_mask_out,
                sd_stream_t stream);
int sd_bn_fold(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
               float eps, int C, float* scale, float* shift, sd_stream_t stream);
/* relu: 0 = none, 1 = ReLU mask from the saved output y, 3 = mask bytes of sd_bn_apply passed as `y`, 2 = mask recomputed from x (layers without a residual
 * input: y is not read at all; needs beta). */
int sd_bn_bwd(const float* dy, const float* x, const float* y, int relu, int64_t M, int C, const float* mean,
              const float* invstd, const float* gamma, const float* beta, float* dx, float* g_out, float* dgamma,
              float* dbeta, int accumulate, void* workspace, size_t workspace_bytes, sd_stream_t stream);
/* out[c] (+)= sum_m x[m][c]  (bias gradients). */
int sd_col_sum(const float* x, int64_t M, int C, float* out, int accumulate, void* workspace,
               size_t workspace_bytes, sd_stream_t stream);

/* MaxPool2d(3, 2, 1) NHWC; idx (uint8 per element) = winning tap for the backward. */
int sd_maxpool3x3s2_fwd(const float* x, float* y, uint8_t* idx, int B, int Hi, int Wi, int C, sd_stream_t stream);
int sd_maxpool3x3s2_bwd(const float* dy, const uint8_t* idx, float* dx, int B, int Hi, int Wi, int C, sd_stream_t stream);
/* Stem tail (network.py:43-45) in training mode, fused: BatchNorm2d (batch statistics given) + ReLU + MaxPool2d(3, 2, 1) straight from
 * the conv output x (B, Hi, Wi, C); the full-resolution activation is never written.  idx as sd_maxpool3x3s2_fwd. */
int sd_bn_relu_maxpool_fwd(const float* x, int B, int Hi, int Wi, int C, const float* mean, const float* invstd, const float* gamma,
                           const float* beta, float* y_pool, uint8_t* idx, sd_stream_t stream);
/* ... and its backward: dpool (B, Ho, Wo, C) -> dx (B, Hi, Wi, C) through max-pool, ReLU and BatchNorm; dgamma / dbeta (+= when
 * accumulate).  workspace = sd_col_reduce_workspace_bytes(B * Hi * Wi, C). */
int sd_maxpool_bn_relu_bwd(const float* dpool, const uint8_t* idx, const float* x, int B, int Hi, int Wi, int C, const float* mean,
                           const float* invstd, const float* gamma, const float* beta, float* dx, float* dgamma, float* dbeta,
                           int accumulate, void* workspace, size_t workspace_bytes, sd_stream_t stream);
/* backward of nn.Upsample(scale_factor=2): dx (B,H,W,C) = 2x2 block sums of dy (B,2H,2W,C) [+ add]. */
int sd_upsample2x_bwd(const float* dy, const float* add, float* dx, int B, int H, int W, int C, sd_stream_t stream);

/* Head (network.py:22-29): 1x1 conv C -> Co with bias; NHWC in, NCHW out (the layout the decoder
 * and the loss consume).  1 <= Co <= SD_HEAD_MAX_CO, i.e. up to 252 labels + parts.
 *   Co <= 32: C = 128 (the default FPN depth), Co <= 16, HW % 16 == 0 and 16-byte aligned pointers take the MFMA kernels (forward:
 *     wave-private LDS-DMA ring + v_mfma_f32_16x16x4_f32; backward: weight-gradient partials likewise, one partial row per wave, before
 *     the data gradient); other shapes the generic kernels (C % 4 == 0, C <= 512 forward; C in {64, 128, 256} backward).
 *   33 <= Co <= 256: C in {64, 128, 256} and B * HW < 2^31, else SD_ERR_INVALID; the forwards need x 16-byte aligned (SD_ERR_ALIGN).
 *     Every pass is a GEMM over the pixels on the MFMA (sd_head_wide.hip): fp32 forward, data gradient and weight-gradient partials on
 *     v_mfma_f32_32x32x2_f32, the bf16 forward on v_mfma_f32_32x32x16_bf16 with the fp32 weights split into two bf16 terms.  Any HW
 *     (ragged tiles are masked).  The workspace holds a fixed number of partial rows that depends on the shape only (at most
 *     about 17 MB; repeated calls give the same bits).
 * Same arithmetic on every path (fp32 products and sums; the order of the sums differs). */
#define SD_HEAD_MAX_CO 256
int sd_head_fwd(const float* x_nhwc, const float* w, const float* bias, float* y_nchw, int B, int HW, int C, int Co,
                sd_stream_t stream);
size_t sd_head_bwd_workspace_bytes(int B, int HW, int C, int Co);
int sd_head_bwd(const float* dy_nchw, const float* x_nhwc, const float* w, float* dx_nhwc, float* dw, float* dbias,
                int B, int HW, int C, int Co, int accumulate, void* workspace, size_t workspace_bytes, sd_stream_t stream);
/* The same with the head's input and its gradient in bf16 (mixed-precision training: no fp32 copies of the FPN output); dy, w, dw, dbias
 * stay fp32.  C in {64, 128}, Co <= 8; same workspace size. */
int sd_head_bwd_bf16(const float* dy, const void* x_bf16, const float* w, void* dx_bf16, float* dw, float* dbias, int B, int HW, int C, int Co,
                     int accumulate, void* workspace, size_t workspace_bytes, sd_stream_t stream);

/* torch.optim.Adam step (defaults: no weight decay / amsgrad) over a flat fp32 buffer;
 * grad is multiplied by grad_scale first (1/world_size after a sum all-reduce). */
int sd_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, int step,
                 float lr, float beta1, float beta2, float eps, float grad_scale, sd_stream_t stream);

/* The same step with the large-batch options (no reference counterpart; the reference's optimizer is plain Adam): decoupled weight decay as
 * in torch.optim.AdamW, global-norm clipping as in torch.nn.utils.clip_grad_norm_, and an exponential moving average of the weights -- one
 * reduction launch (only for clipping) plus one fused update, no host synchronisation.
 *   sd_grad_sumsq: fp64 partial sums of squares of grad[0..n) into the workspace (sd_grad_sumsq_workspace_bytes(n) bytes = one double per
 *     block, 8-byte aligned; every one is written, earlier contents do not matter).  Fixed reduction order: the same gradients give the same
 *     bits on every run and on every rank.
 *   sd_optim_step: sd_adam_step's arguments, then
 *     weight_decay >= 0 and decay_mask: p *= 1 - lr * weight_decay before the Adam update where decay_mask[i / 4] != 0 (one byte per group of
 *       four floats; NULL: everywhere);
 *     max_norm >= 0 (0: no clipping), partials / npartials: the workspace sd_grad_sumsq has just filled and its count of doubles.  Every
 *       block finishes the partials itself in fp64 in a fixed order: norm = |grad_scale| * sqrt(sum) is the norm of the gradient after
 *       grad_scale, the gradient is multiplied by min(1, max_norm / (norm + 1e-6)).  A norm that is not finite (an inf or nan gradient) skips
 *       the step: parameters, moments and EMA are not written;
 *     ema (NULL: none) and ema_decay in [0, 1): ema = ema_decay * ema + (1 - ema_decay) * p_new, from the registers holding the new parameter;
 *     status (SD_OPTIM_STATUS_BYTES, 4-byte aligned; needed and written only when max_norm > 0): [0] float norm, [1] float coefficient applied
 *       (0 for a skipped step), [2] int32 count of skipped steps (incremented, never reset), [3] reserved.
 *   Options that are off are compiled out (one kernel per combination); with all three off the launch is sd_adam_step's own kernel.
 * Errors (text in sd_last_error()): SD_ERR_INVALID for n % 4 != 0, step < 1, negative weight_decay / max_norm, ema_decay outside [0, 1),
 * max_norm > 0 without partials or status; SD_ERR_ALIGN for misaligned pointers; SD_ERR_WORKSPACE for a workspace that is too small. */
#define SD_OPTIM_STATUS_BYTES 16
size_t sd_grad_sumsq_workspace_bytes(int64_t n);
int sd_grad_sumsq(const float* grad, int64_t n, void* workspace, size_t workspace_bytes, sd_stream_t stream);
int sd_optim_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, int step,
                  float lr, float beta1, float beta2, float eps, float grad_scale, float weight_decay,
                  const uint8_t* decay_mask, float max_norm, const void* partials, int npartials, float* ema,
                  float ema_decay, void* status, sd_stream_t stream);

/* sd_optim_step with a learning rate and a weight decay per parameter GROUP (fine-tuning: a lower rate on the pretrained trunk, layer-wise
 * rate decay) -- still one update launch over the whole flat buffer.  sd_optim_step's arguments, with the decay mask replaced by
 *   group_ids (device, required): one byte per group of four floats (n / 4 bytes), laid out like decay_mask -- a group of four never
 *     straddles two tensors.  The kernel uses id & 15: a stray byte cannot read outside the table, it names a row; the ids are not scanned;
 *   lr_mul, wd_mul (HOST arrays of ngroups floats, 1 <= ngroups <= SD_OPTIM_MAX_GROUPS, every entry finite and >= 0): read during the call
 *     and handed to the kernel by value in its arguments -- no device table, no upload, no lifetime rule.  Group k steps with
 *     lr_k = lr * lr_mul[k] (one float multiply) and is decayed by p *= (float)(1 - (double)lr_k * weight_decay * wd_mul[k]) before the
 *     update; wd_mul[k] == 0 or weight_decay == 0: group k is not decayed.  Rows k >= ngroups are 0 / 0: such a group does not move.
 *     lr_mul[k] == 0 is torch's lr = 0 group: moments and EMA still update, the parameter does not move.
 * Everything else is sd_optim_step's update in its operation order: a table [1, 1] / [0, 1] over ids equal to a 0 / 1 decay mask gives
 * sd_optim_step's bits.  Clipping (the GLOBAL norm over all groups, from the same sd_grad_sumsq partials; a non-finite norm skips the step
 * for every group), EMA and the status block behave exactly as there.  One kernel per (clipping, EMA) combination; decay is decided per
 * group from the table.
 * Errors: sd_optim_step's, and SD_ERR_INVALID for a null group_ids / lr_mul / wd_mul, ngroups outside 1 .. 16, a negative or non-finite
 * multiplier. */
#define SD_OPTIM_MAX_GROUPS 16
int sd_optim_groups_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, int step,
                         float lr, float beta1, float beta2, float eps, float grad_scale, float weight_decay,
                         const uint8_t* group_ids, const float* lr_mul, const float* wd_mul, int ngroups,
                         float max_norm, const void* partials, int npartials, float* ema, float ema_decay,
                         void* status, sd_stream_t stream);

/* The other two update rules over the same flat buffers (`train --optimizer sgd|lamb`; no reference counterpart, no accuracy claim: the
 * deliverable is the update rule).  Both take the GROUPS form of sd_optim_groups_step: group_ids (device, one byte per group of four floats,
 * id & 15), the HOST tables lr_mul / wd_mul by value (ngroups entries; a uniform table = no per-stage rates), grad_scale, max_norm +
 * partials / npartials from sd_grad_sumsq (the GLOBAL norm; a non-finite norm skips the whole step: no launch of the step writes anything
 * but status[0..2], and status[2] goes up by one), ema / ema_decay, status -- same meaning, same refusals and codes.  Group k steps with
 * lr_k = lr * lr_mul[k] and wd_k = weight_decay * wd_mul[k] (one float multiply each).
 *
 * sd_sgd_step: torch.optim.SGD with dampening 0, one launch (sd_optim_groups_step's traffic minus one moment buffer), per element
 *     d = grad * grad_scale * clip_coef;  if wd_k > 0: d += wd_k * p
 *     if momentum > 0: buf = momentum * buf + d;  d = nesterov ? d + momentum * buf : buf
 *     p -= lr_k * d;  ema = ema_decay * ema + (1 - ema_decay) * p_new
 *   The decay is COUPLED L2 (it enters the gradient, and through it the momentum), as in torch.optim.SGD -- not AdamW's decoupled decay of
 *   sd_optim_step.  A zero buffer at step 1 gives torch's buf = d.  momentum == 0: the buffer is neither read nor written and may be NULL.
 *   Errors, beyond the groups form's: SD_ERR_INVALID for momentum outside [0, 1), nesterov outside 0 / 1 or with momentum == 0, a null
 *   buffer with momentum > 0.
 *
 * sd_lamb_step: LAMB (You et al. 2020, Alg. 2), two launches, per parameter SLOT s and its groups k
 *     g = grad * grad_scale * clip_coef;  m = beta1 * m + (1 - beta1) * g;  v = beta2 * v + (1 - beta2) * g * g
 *     u = (m / (1 - beta1^t)) / (sqrt(v) / sqrt(1 - beta2^t) + eps) + wd_k * p
 *     phi_s = adapt_s and |p_s| > 0 and |u_s| > 0 and both finite ? |p_s| / |u_s| : 1      (L2 norms over the slot, p BEFORE the update)
 *     p -= lr_k * phi_s * u;  ema as above
 *   Which slots adapt is the table's bit, set by the caller; `Network.optim_slots()` sets it for 4-D tensors (convolution weights) whatever
 *   weight_decay is, and leaves biases and BatchNorm weight / bias at phi = 1.  (apex FusedLAMB ties the exclusion to weight_decay == 0
 *   instead: there a run without decay adapts nothing unless use_nvlamb is set.)  lr_mul[k] == 0: moments and EMA update, p does not move.
 *   The slot table is static per network: sd_lamb_table_build (host only, no HIP call) lays it out from the slot ranges -- the slots must
 *   tile [0, n) in order, each a positive multiple of 8 floats -- and reports its size and the block count; with table == NULL it only
 *   reports.  The caller uploads the table once (16-byte aligned) and hands it to every step with nslots and nblocks.  Layout (int32):
 *   [nslots][4] = {lo / 4, hi / 4, first block, block count | adapt << 30}, then [nblocks] slot indices.  A slot of f floats gets
 *   min(ceil(f / SD_LAMB_BLOCK_FLOATS), SD_LAMB_MAX_SLOT_BLOCKS) blocks; no block works on two slots.  The kernels clamp every value they
 *   read from the table into [0, n / 4) and [0, nblocks): a wrong table gives wrong numbers, never an access outside the buffers.
 *   Pass 1 (k_lamb_moments) writes m, v and one fp64 (sum p^2, sum u^2) pair per block into the workspace (sd_lamb_workspace_bytes(nblocks),
 *   8-byte aligned, every pair written: earlier contents do not matter); pass 2 (k_lamb_apply): every block finishes its slot's pairs itself,
 *   recomputes u from the stored m, v and p, and applies.  Both norms are fp64 sums in a fixed order (per thread in index order, lanes by
 *   shuffle, waves in order, a slot's blocks in block order), no atomics: the same inputs give the same bits on every run and every rank.
 *   Errors, beyond the groups form's: SD_ERR_INVALID for step < 1, null moments / table / workspace, nslots outside [1, SD_LAMB_MAX_SLOTS],
 *   nblocks outside [nslots, SD_LAMB_MAX_SLOT_BLOCKS * nslots], n >= 2^33; SD_ERR_ALIGN; SD_ERR_WORKSPACE for a workspace (or, in the
 *   builder, a table) that is too small.  sd_lamb_table_build: SD_ERR_INVALID for null arrays, a slot count out of range, slots that do
 *   not tile [0, n). */
#define SD_LAMB_BLOCK_FLOATS 4096
#define SD_LAMB_MAX_SLOT_BLOCKS 128
#define SD_LAMB_MAX_SLOTS 65536
int sd_sgd_step(float* param, const float* grad, float* momentum_buf, int64_t n, float lr, float momentum, int nesterov,
                float grad_scale, float weight_decay, const uint8_t* group_ids, const float* lr_mul, const float* wd_mul,
                int ngroups, float max_norm, const void* partials, int npartials, float* ema, float ema_decay,
                void* status, sd_stream_t stream);
size_t sd_lamb_workspace_bytes(int nblocks);
int sd_lamb_table_build(const int64_t* slot_lo, const int64_t* slot_hi, const uint8_t* adapt, int nslots, int64_t n,
                        void* table, size_t table_bytes, size_t* bytes_needed, int* nblocks);
int sd_lamb_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, int step,
                 float lr, float beta1, float beta2, float eps, float grad_scale, float weight_decay,
                 const uint8_t* group_ids, const float* lr_mul, const float* wd_mul, int ngroups,
                 float max_norm, const void* partials, int npartials, float* ema, float ema_decay, void* status,
                 const void* table, int nslots, int nblocks, void* workspace, size_t workspace_bytes, sd_stream_t stream);

/* Gradient accumulation (`train --accum_steps K`): one streaming launch that folds a micro-batch's gradient into a running sum.
 *   overwrite = 0: dst[i] = dst[i] + src[i] -- one fp32 add per element, no FMA, no rescaling: the bits of torch's `dst += src`;
 *   overwrite = 1: dst[i] = src[i] (the first micro-batch of a group: no zero-fill pass before it).
 * In place on dst, on the caller's stream; no workspace, no atomics.  The mean is taken later, by the optimizer's grad_scale
 * (1 / (k * world) for a group of k micro-batches).  n floats, n % 4 == 0; n == 0 succeeds without a launch (and reads no pointer).  dst and
 * src may be the same range; any other overlap is refused.
 * Errors: SD_ERR_INVALID for n < 0, n % 4 != 0, a null pointer with n > 0, overwrite outside 0 / 1, partially overlapping ranges;
 * SD_ERR_ALIGN for a pointer that is not 16-byte aligned. */
int sd_grad_accum(float* dst, const float* src, int64_t n, int overwrite, sd_stream_t stream);

/* What a call of the BatchNorm / pool / head / optimizer entry points above launches (host only; no pointer is read).  The descriptor names
 * the call: `op`, `form` (0 fp32, 1 bf16, 2 bf16 with a bf16 dx -- the stem tail's _dx16; SD_NN_CAST: 0 = to bf16, 1 = to fp32), the shape
 * (the map ops take B, H, W; the head B and H = HW; every other op M -- the optimizer and the casts their n), C, Co, relu, rows (the
 * caller-provided-rows forms) and `flags`: bit k (k < 4) = pointer k of the op's kernel choice is 16-byte aligned, in the order
 *     bn_apply: x, y, residual        bn_bwd / bn_bwd_apply: dy, x, dx, g_out (bn_bwd_reduce: dy, x)        bn_relu_maxpool_fwd: x, y_pool, idx
 *     head_fwd: x, w, y               head_bwd: x, dy
 * SD_NN_SCRATCH = scratch given, SD_NN_SUMS = the split form that stops at the fp64 sums (sd_bn_train_sums, sd_bn_stats_sums, sd_bn_bwd_sums,
 * sd_bn_bwd_reduce, sd_maxpool_bn_relu_bwd_reduce), SD_NN_DECAY / _CLIP / _EMA = the options of sd_optim_step (_CLIP / _EMA: of sd_optim_groups_step, sd_sgd_step and sd_lamb_step too).  pool_fwd_pair: the option
 * of that name as the call would see it.
 * sd_nn_kernel_names prints the launches in order, separated by "; ", each as "<kernel as rocprofv3 prints it, without sd::> grid=X block=256
 * lds=N" (N: dynamic bytes), a wide head's own kernels as "head_wide_fwd" / "head_wide_wgrad" / "head_wide_dgrad" (their grids need the
 * device).  Reducing ops append " | rpb=.. nb=.. slab=.. rows=.. partial_at=.. means_at=.. fold_at=.. ws_bytes=.." (slab 0 = no fold; rows =
 * what the finish reads; offsets in floats), the caller-provided-rows forms " | slab=.. rows=..", the head backward and sd_grad_sumsq
 * " | ws_bytes=..".  "refused: <message>" for an unknown op and where one of the layer's shared shape checkers refuses the call: C (and M) of
 * the BatchNorm / column-sum / stem-tail family, relu outside 0..3, the map checks of the pool and upsample entry points, a bf16 stem tail on
 * an odd map, n % 4 != 0 of the casts, the optimizer and sd_grad_accum (and its form outside 0 / 1).  The checks an entry point states for itself are not asked -- the head's limits on
 * C and Co (the query prints the launches of the form the descriptor names), rows <= 0, null pointers, workspace sizes.  A refusal sets
 * sd_last_error() of the calling thread, as the entry point's own would; an answered query leaves it alone.  The answer is made from the
 * plans, launch shapes and predicates the launchers themselves run.  Thread-local storage, valid until the next call on the thread. */
enum { SD_NN_BN_TRAIN_STATS, SD_NN_BN_FINALIZE_STATS, SD_NN_BN_STATS_FROM_SUMS, SD_NN_BN_APPLY, SD_NN_BN_FOLD, SD_NN_BN_BWD, SD_NN_BN_BWD_REDUCE,
       SD_NN_BN_BWD_FINALIZE, SD_NN_BN_BWD_MEANS_FROM_SUMS, SD_NN_BN_BWD_APPLY, SD_NN_COL_SUM, SD_NN_MAXPOOL_FWD, SD_NN_MAXPOOL_BWD,
       SD_NN_BN_RELU_MAXPOOL_FWD, SD_NN_STEM_BWD, SD_NN_STEM_BWD_REDUCE, SD_NN_STEM_BWD_APPLY, SD_NN_UPSAMPLE_BWD, SD_NN_CAST, SD_NN_HEAD_FWD,
       SD_NN_HEAD_BWD, SD_NN_ADAM, SD_NN_GRAD_SUMSQ, SD_NN_OPTIM,
       /* ops 0 .. 23 are the ones of the recorded call trace (tests/golden/nn_call_trace.json), and 24, the first id behind them, is the
        * one tests/test_nn_plan_cpu.py asks about as an unknown op: it stays unused, ops added since follow from 25.  bn_frozen_bwd (sd_frozen_bn_bwd[_bf16]): M, C, form; flag bits: dy, y, dx, g_out
        * (a pointer the call leaves NULL counts as aligned) */
       SD_NN_BN_FROZEN_BWD = 25,
       /* sd_optim_groups_step: n in M; flags SD_NN_CLIP / SD_NN_EMA.  Prints the step's launches: k_grad_sumsq (with SD_NN_CLIP: the
        * sd_grad_sumsq call that feeds it), then k_optim_groups<clip, ema> */
       SD_NN_OPTIM_GROUPS = 26,
       /* sd_grad_accum: n in M; form 0 = add (k_grad_accum<false>), 1 = overwrite (k_grad_accum<true>); n == 0: no launch, an empty answer.
        * 27 is skipped as 24 is: tests/test_optim_groups_cpu.py asks about both as unknown ops, so they stay unused */
       SD_NN_GRAD_ACCUM = 28,
       /* 29 is skipped as 24 and 27 are (tests/test_accum_cpu.py asks about it as an unknown op).  The step's calls of the two other
        * optimizers, n in M, flags SD_NN_CLIP / SD_NN_EMA as for SD_NN_OPTIM_GROUPS; both print k_grad_sumsq first with SD_NN_CLIP.
        * sd_sgd_step: form 0 = no momentum, 1 = momentum, 2 = Nesterov; k_sgd<form, clip, ema> on sd_adam_step's grid.
        * sd_lamb_step: the grid depends on the slot table, so the query takes sd_lamb_table_build's block count in `rows` (rows < 1 is
        * refused): k_lamb_moments<clip> and k_lamb_apply<clip, ema>, both grid = rows, then " | ws_bytes=.." (sd_lamb_workspace_bytes(rows)) */
       SD_NN_SGD = 30, SD_NN_LAMB = 31 };
#define SD_NN_SCRATCH (1u << 8)
#define SD_NN_SUMS (1u << 9)
#define SD_NN_DECAY (1u << 10)
#define SD_NN_CLIP (1u << 11)
#define SD_NN_EMA (1u << 12)
typedef struct {
    int op, form, B, H, W;
    int64_t M;
    int C, Co, relu, rows;
    unsigned flags;
    int pool_fwd_pair;
} sd_nn_call_desc;
const char* sd_nn_kernel_names(const sd_nn_call_desc* d);

/* ---- gradient exchange (the reference's step, trainer.py:113-124, is single-device) -------------------
 * Thin wrapper over RCCL, one communicator per process (= per GPU).  librccl.so.1 is dlopen()ed on first use (the copy a
 * PyTorch-ROCm process has already loaded is reused), so libsdnet_hip.so has no link-time dependency on it.
 * Bootstrap: rank 0 calls sd_allreduce_unique_id and hands the 128 bytes to the other ranks by any host channel
 * (torch.distributed store, MPI, a file); every rank then calls sd_allreduce_init with the device it computes on current.
 * sd_allreduce_run: in-place fp32 sum over all ranks of buf[0..count), asynchronous on `stream`.  Positive return values of
 * these four functions are ncclResult_t codes (text in sd_last_error()). */
#define SD_COMM_ID_BYTES 128
int sd_allreduce_unique_id(void* id_out);
int sd_allreduce_init(const void* id, int rank, int world, void** comm_out);
int sd_allreduce_run(void* comm, float* buf, int64_t count, sd_stream_t stream);
int sd_allreduce_destroy(void* comm);

/* Stand-in for ONE RCCL all-reduce launch on a single GPU (no reference counterpart; sizing tool for the data-parallel step, csrc/sd_commsim.hip):
 * `workgroups` persistent blocks of 256 threads / 8 KB LDS copy `move_bytes` (a multiple of 16; the source of `src_bytes` wraps) from src to dst,
 * throttled on the 100 MHz wall clock to `gbps` GB/s in total -- the launch occupies its CUs for move_bytes / gbps like a link-bound collective.
 * `TrainStep(exchange="sim")` issues it at the five bucket trigger points of the backward on the exchange's side stream; bench.py reports the
 * step time with and without it (`north_star.comm_sim`). */
int sd_comm_sim_copy(const void* src, void* dst, size_t src_bytes, size_t move_bytes, int workgroups, float gbps, sd_stream_t stream);

/* The box's own bf16 MFMA ceiling (no reference counterpart; measurement, csrc/sd_bench.hip): 256 blocks x 512 threads run `iters` K = 32
 * steps of a bare LDS-read + v_mfma_f32_16x16x32_bf16 loop (wave tile 128 x 64, the bf16 conv kernels' shape) on the 64 KB of bf16 operands at
 * `operands64k`; `out` receives 256 x 512 floats (so that nothing is optimised away).  sd_mfma_bf16_stream_flops(iters) = the flop count of one
 * launch; bench.py times warm launches with stream events and reports the bf16 forwards as a fraction of that rate beside the nominal peak. */
double sd_mfma_bf16_stream_flops(int iters);
int    sd_mfma_bf16_stream(const void* operands64k, float* out, int iters, sd_stream_t stream);

/* ---- synchronized BatchNorm (data-parallel training: statistics over the whole global batch) ----
 * Every batch-statistics finish above is one launch that reduces partial rows to per-channel sums in double, in a fixed order, and
 * turns them into outputs.  The split forms below stop after the first half and hand the sums to the caller in ONE fp64 vector
 *     sums = [S0 (C), S1 (C), n]      forward:  S0 = sum x,  S1 = sum x^2;   backward: S0 = sum g,  S1 = sum g * xhat
 * (n = the element count M of this call, C + C + 1 doubles, 8-byte aligned), so that the caller can all-reduce it (sum) across ranks;
 * the second half then turns the (global) sums into outputs.  Summation order and arithmetic are those of the one-launch finish: with
 * no exchange in between, split == fused bit for bit.  The backward's phase 1 writes dgamma / dbeta (+= when accumulate) from the
 * LOCAL sums (they reach the other ranks through the gradient all-reduce).  Workspaces are those of the fused forms.
 * These are contract changes (results depend on what the caller does with `sums`), hence explicit entry points, not sd_set_option. */
/* phase 2, forward: mean = S0/n, invstd = 1/sqrt(S1/n - mean^2 + eps), running stats with momentum and the unbiased var
 * (var * n/(n-1)); running_mean / running_var both given or both null.  Phase 2, backward: means_out = [S0/n (C), S1/n (C)] as
 * sd_bn_bwd_apply / sd_bn_bwd_apply_bf16 / sd_maxpool_bn_relu_bwd_apply* consume them. */
int sd_bn_stats_from_sums(const double* sums, int C, float eps, float momentum, float* running_mean, float* running_var, float* mean,
                          float* invstd, sd_stream_t stream);
int sd_bn_bwd_means_from_sums(const double* sums, int C, float* means_out, sd_stream_t stream);
/* phase 1 of sd_bn_finalize_stats / sd_bn_bwd_finalize on caller-provided partial rows (same rows, scratch and order) */
int sd_bn_stats_sums(const float* partial, int rows, int64_t M, int C, double* sums, float* scratch, sd_stream_t stream);
int sd_bn_bwd_sums(const float* partial, int rows, int64_t M, int C, float* dgamma, float* dbeta, int accumulate, double* sums,
                   float* scratch, sd_stream_t stream);
/* sd_bn_train_stats[_bf16] stopping after phase 1 */
int sd_bn_train_sums(const float* x, int64_t M, int C, double* sums, void* workspace, size_t workspace_bytes, sd_stream_t stream);
int sd_bn_train_sums_bf16(const void* x, int64_t M, int C, double* sums, void* workspace, size_t workspace_bytes, sd_stream_t stream);
/* the fused conv forwards stopping after phase 1 (the statistics still come from the conv epilogue: no extra pass over y).
 * sd_conv2d_fwd_bn_stats_rows: partial rows the epilogue of that forward writes (bf16 = 0: fp32 kernels, 1: bf16 kernels);
 * 0 = the split-K two-pass form (conv, then sd_bn_train_stats); -1 = unsupported geometry.  Host arithmetic only. */
int sd_conv2d_fwd_bn_stats_rows(const sd_conv_desc* d, int bf16);
int sd_conv2d_fwd_bn_sums(const float* x, const float* w, float* y, const sd_conv_desc* d, double* sums, void* workspace,
                          size_t workspace_bytes, sd_stream_t stream);
int sd_conv2d_fwd_bf16_bn_sums(const void* x, const void* w, void* y, const sd_conv_desc* d, double* sums, void* workspace,
                               size_t workspace_bytes, sd_stream_t stream);
int sd_conv2d_stem_fwd_bn_sums(const float* x_nchw, const float* w, float* y, const sd_conv_desc* d, double* sums, void* workspace,
                               size_t workspace_bytes, sd_stream_t stream);
int sd_conv2d_stem_fwd_bn_sums_bf16mm(const float* x_nchw, const float* w, float* y, const sd_conv_desc* d, double* sums, void* workspace,
                                      size_t workspace_bytes, sd_stream_t stream);
int sd_conv2d_stem_fwd_bn_sums_bf16(const float* x_nchw, const float* w, void* y_bf16, const sd_conv_desc* d, double* sums, void* workspace,
                                    size_t workspace_bytes, sd_stream_t stream);
/* the fused data-gradient + BatchNorm-backward reduction stopping after phase 1 (dgamma / dbeta += local sums) */
int sd_conv2d_dgrad_bn_reduce_sums(const float* dy, const float* w_t, float* dx, const sd_conv_desc* d, const float* residual,
                                   const float* bn_x, const float* bn_y, int relu, const float* mean, const float* invstd,
                                   const float* gamma, const float* beta, float* dgamma, float* dbeta, int accumulate,
                                   double* sums, void* workspace, size_t workspace_bytes, sd_stream_t stream);
/* the reduce half of sd_bn_bwd[_bf16] (relu as there); the apply half is sd_bn_bwd_apply / sd_bn_bwd_apply_bf16 (the bf16 forms
 * choose their 8-wide kernels from 16-byte alignment as sd_bn_bwd_bf16 does: buffers of one allocator make the same choice) */
int sd_bn_bwd_reduce(const float* dy, const float* x, const float* y, int relu, int64_t M, int C, const float* mean, const float* invstd,
                     const float* gamma, const float* beta, float* dgamma, float* dbeta, int accumulate, double* sums, void* workspace,
                     size_t workspace_bytes, sd_stream_t stream);
int sd_bn_bwd_reduce_bf16(const void* dy, const void* x, const void* y, int relu, int64_t M, int C, const float* mean, const float* invstd,
                          const float* gamma, const float* beta, float* dgamma, float* dbeta, int accumulate, double* sums, void* workspace,
                          size_t workspace_bytes, sd_stream_t stream);
int sd_bn_bwd_apply_bf16(const void* dy, const void* x, const void* y, int relu, int64_t M, int C, const float* mean, const float* invstd,
                         const float* gamma, const float* beta, const float* means, void* dx, void* g_out, sd_stream_t stream);
/* the stem tail's backward in two halves: reduce (sd_maxpool_bn_relu_bwd's reduction + phase 1; fp32, or bf16 dpool / x) and apply
 * from the means of sd_bn_bwd_means_from_sums (fp32; bf16 in, fp32 dx; bf16 in, bf16 dx).  Workspace as sd_maxpool_bn_relu_bwd. */
int sd_maxpool_bn_relu_bwd_reduce(const float* dpool, const uint8_t* idx, const float* x, int B, int Hi, int Wi, int C, const float* mean,
                                  const float* invstd, const float* gamma, const float* beta, float* dgamma, float* dbeta, int accumulate,
                                  double* sums, void* workspace, size_t workspace_bytes, sd_stream_t stream);
int sd_maxpool_bn_relu_bwd_reduce_bf16(const void* dpool_bf16, const uint8_t* idx, const void* x_bf16, int B, int Hi, int Wi, int C,
                                       const float* mean, const float* invstd, const float* gamma, const float* beta, float* dgamma,
                                       float* dbeta, int accumulate, double* sums, void* workspace, size_t workspace_bytes, sd_stream_t stream);
int sd_maxpool_bn_relu_bwd_apply(const float* dpool, const uint8_t* idx, const float* x, int B, int Hi, int Wi, int C, const float* mean,
                                 const float* invstd, const float* gamma, const float* beta, const float* means, float* dx, sd_stream_t stream);
int sd_maxpool_bn_relu_bwd_apply_bf16(const void* dpool_bf16, const uint8_t* idx, const void* x_bf16, int B, int Hi, int Wi, int C,
                                      const float* mean, const float* invstd, const float* gamma, const float* beta, const float* means, float* dx,
                                      sd_stream_t stream);
int sd_maxpool_bn_relu_bwd_apply_bf16_dx16(const void* dpool_bf16, const uint8_t* idx, const void* x_bf16, int B, int Hi, int Wi, int C,
                                           const float* mean, const float* invstd, const float* gamma, const float* beta, const float* means,
                                           void* dx_bf16, sd_stream_t stream);

/* ---- frozen BatchNorm, backward (fine-tuning: `Network.freeze`) ----------------------------------------------------
 * A BatchNorm that normalises with its stored statistics is the per-channel affine y = x * scale[c] + shift[c] (sd_bn_fold), so its
 * backward has no reduction:  g = (y == NULL || y[i] > 0) ? dy[i] : +0;  g_out[i] = g;  dx[i] = g * scale[i % C]  (one fp32 multiply;
 * the bf16 form: g_out = dy's bits or +0, dx = round-to-nearest-even(float(g) * scale[c])).  y: the layer's ReLU output or NULL (no ReLU);
 * g_out: NULL or the masked gradient (what the skip path of a residual block takes).  A pure function of its inputs: one launch, no
 * workspace, no atomics, grid-stride over any M.  C as the BatchNorm family (C % 4 == 0 ...), M >= 1; dx and g_out must not alias
 * dy, y or each other (SD_ERR_INVALID).  16-byte loads and stores where every pointer given is 16-byte aligned (the bf16 form: and
 * C % 8 == 0), element-wise ones otherwise.  Named sd_frozen_bn_* (not sd_bn_frozen_*): the sd_bn_* names are the entry points of the
 * recorded call trace (tests/golden/nn_call_trace.json), which this one came after. */
int sd_frozen_bn_bwd(const float* dy, const float* y, const float* scale, int64_t M, int C, float* dx, float* g_out, sd_stream_t stream);
int sd_frozen_bn_bwd_bf16(const void* dy, const void* y, const float* scale, int64_t M, int C, void* dx, void* g_out, sd_stream_t stream);

/* ---- profiler ranges (no reference counterpart: SURVEY.md section 5 lists tracing as absent from the reference) ----
 * roctx ranges on the calling thread, for `rocprofv3 --marker-trace`.  Active only when the environment holds SDNET_ROCTX=1 at the
 * first call AND a marker library (librocprofiler-sdk-roctx / libroctx64) can be dlopen'ed; otherwise every call is a no-op returning 0.
 * sd_range_enabled: 1 when ranges are recorded.  sd_range_library: the soname that was loaded ("" when disabled).
 * The host mirror (structuredetector_amd/utils/trace.py) brackets target rendering, the forward stages, the loss, the backward stages,
 * every gradient bucket and the Adam launch of `TrainStep` with them. */
int         sd_range_enabled(void);
const char* sd_range_library(void);
int         sd_range_push(const char* name);
int         sd_range_pop(void);
int         sd_range_mark(const char* name);

#ifdef __cplusplus
}
#endif
#endif /* SDNET_HIP_H */
