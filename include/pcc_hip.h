/*
 * libpcc_hip.so — C-ABI of the MI355X-native encode/decode operators of the joint
 * geometry+attribute point-cloud codec (ColorModel.compress / decompress / forward).
 *
 * The reference (/root/reference) has no FFI of its own: its operators are Python calls
 * into MinkowskiEngine (model/model.py:3, model/transforms.py:3, model/blocks.py:3,
 * model/entropy_models.py:5) and compressai (model/entropy_models.py:9-10).  Each entry
 * point below names the reference call site(s) it replaces.  INTEGRATION.md shows the
 * ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *   - plain pointers and sizes only; device pointers unless marked "host".
 *   - all buffers are caller-owned (torch tensors on the Python side); the library never
 *     allocates device memory.  `stream` is a hipStream_t passed as void*.
 *   - every function returns 0 on success or a negative PCC_ERR_* code; the message is
 *     available from pcc_last_error() (thread-local).  No exceptions cross the ABI.
 *   - coordinates: int32 [N,4] rows (batch, x, y, z), |x|,|y|,|z| <= PCC_COORD_LIMIT, batch <= PCC_BATCH_LIMIT.
 *   - features: fp32 row-major [N, C].  Neighbour tables: int32 [N_out, K], -1 = absent.
 *   - hash table = (keys uint64[cap], vals int32[cap], tensor_stride), cap a power of two from
 *     pcc_hash_capacity(); a table is immutable once built and may be read concurrently.
 *     `tensor_stride` is the grid pitch of the coordinate set the table indexes (every coordinate a
 *     multiple of it; 1 for arbitrary integer coordinates): the slot function keeps 8 grid steps
 *     along z in one cache line, so build and every later probe must name the same value (any
 *     value >= 1 is correct, the set's own stride is the fast one).  pcc_stride_map / pcc_children /
 *     pcc_kernel_map derive it from their `ts` / `step` arguments.
 */
#ifndef PCC_HIP_H
#define PCC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCC_OK 0
#define PCC_ERR_ARG (-1)
#define PCC_ERR_HIP (-2)
#define PCC_ERR_UNSUPPORTED (-3)
#define PCC_ERR_DATA (-4)

#define PCC_ACT_NONE 0
#define PCC_ACT_RELU 1       /* ME.MinkowskiReLU */
#define PCC_ACT_LEAKY_RELU 2 /* ME.MinkowskiLeakyReLU, slope 0.01 */

int pcc_version(void);
const char* pcc_last_error(void);
/* Number of devices visible to the library and a short name of device `dev` (host). */
int pcc_device_count(void);
int pcc_device_name(int dev, char* out, int out_len);

/* ---------------------------------------------------------------------------------------
 * Coordinate manager (ME coordinate_map_*; every ME.SparseTensor(...) construction, e.g.
 * model/model.py:59,64,122,188).
 * ------------------------------------------------------------------------------------- */
int64_t pcc_hash_capacity(int64_t n);

/* Coordinate range.  A voxel key has 10 bits of batch index and 18 bits per coordinate: coordinates must satisfy
 * |c| <= PCC_COORD_LIMIT and batch indices 0 <= b <= PCC_BATCH_LIMIT — the reference's radix-1e5 keys (model/blocks.py:118 and
 * utils.py:170: coordinates 0 .. 99,999) fit, with the same span on the negative side.  A set with a coordinate outside the
 * range is never hashed with an aliased key: pcc_stride_map / pcc_children check the source rows and every generated
 * coordinate and report *out_count = PCC_COUNT_ERR_RANGE instead of a row count — the error reaches the host with the one
 * value it reads anyway, at no extra synchronisation (the Python side raises ValueError). */
#define PCC_COORD_LIMIT 130000
#define PCC_BATCH_LIMIT 1022
#define PCC_COUNT_ERR_RANGE (-2)

/* Insert rows 0..n-1; table value = row index.  Duplicate coordinates keep the smallest
 * row index and increment *dup_count (device int32, may be NULL). */
int pcc_hash_build(const int32_t* coords, int64_t n, uint64_t* keys, int32_t* vals, int64_t cap,
                   int32_t tensor_stride, int32_t* dup_count, void* stream);

/* out_idx[i] = row of query i or -1.  A query with a coordinate beyond PCC_COORD_LIMIT or a batch index outside
 * 0 .. PCC_BATCH_LIMIT is in no set: it gets -1, never the row of the voxel its masked key would alias.
 * (features_at_coordinates on on-grid integer queries:
 * model/transforms.py:96,124,262; model/blocks.py:37,50; model/entropy_models.py:326,364,401;
 * torch.isin of model/blocks.py:125.) */
int pcc_hash_lookup(const uint64_t* keys, const int32_t* vals, int64_t cap, int32_t tensor_stride,
                    const int32_t* query, int64_t nq, int32_t* out_idx, void* stream);

/* Scratch (int32 elements) needed by pcc_stride_map / pcc_children / pcc_compact_* for m candidates. */
int64_t pcc_scan_scratch_elems(int64_t m);

/* Output coordinate set of a stride-2 convolution on a tensor of stride `ts`
 * (ME stride map; model/transforms.py:49-51, model/blocks.py:203,
 * model/entropy_models.py:276,280, model/model.py:189-190):
 * unique floor(c / 2ts) * 2ts, in order of first appearance.  out_coords has room for n
 * rows; *out_count (device int64) receives the number of unique rows, or
 * PCC_COUNT_ERR_RANGE if a source or output coordinate is outside the key range.  On return
 * (keys, vals, cap) is the hash table of the OUTPUT set (cap >= pcc_hash_capacity(n)). */
int pcc_stride_map(const int32_t* coords, int64_t n, int32_t ts, uint64_t* keys, int32_t* vals,
                   int64_t cap, int32_t* scratch, int32_t* out_coords, int64_t* out_count,
                   void* stream);

/* Output coordinate set of a generative transposed convolution, kernel `ksize` (2 or 3),
 * stride 2, on a tensor of stride `ts` (ME.MinkowskiGenerativeConvolutionTranspose:
 * model/blocks.py:84, model/entropy_models.py:286,290; ConvolutionTranspose :298,302):
 * unique c + off_k * ts/2.  Candidates are enumerated parent-major for ksize 3 and
 * offset-major for ksize 2; the output keeps first appearances in that order.
 * out_coords has room for n * ksize^3 rows; table as in pcc_stride_map
 * (cap >= pcc_hash_capacity(n * ksize^3)). */
int pcc_children(const int32_t* coords, int64_t n, int32_t ts, int32_t ksize, uint64_t* keys,
                 int32_t* vals, int64_t cap, int32_t* scratch, int32_t* out_coords,
                 int64_t* out_count, void* stream);

/* ---------------------------------------------------------------------------------------
 * Training augmentation (data/transform.py of the reference; every configuration applies both,
 * configs/Ours.yaml:29-35).
 * ------------------------------------------------------------------------------------- */
/* RandomRotate (data/transform.py:425-494) for a whole collated batch: every row is rotated about the
 * block centre by the matrix of its batch item, rounded to the voxel grid, and duplicates are dropped.
 * rot: float32 [nbatch,9], row-major 3x3 per item; half = block_size / 2.  The arithmetic is exact fp32,
 * every product and sum rounded separately (numpy float32 reproduces it bit for bit):
 *     d = (float)c - half                                  per axis
 *     x' = ((d_x R00 + d_y R01) + d_z R02) + half          rows 1 and 2 of R alike for y', z'
 *     rintf (ties to even), then the conversion to int32;  the batch index passes through
 * which is the sum order of torch.mm(points - s/2, R.T) + s/2.  With the identity matrix integer
 * coordinates pass through unchanged.  Candidates that land on the same (batch, x, y, z) keep the lowest
 * input row; output rows come in input order of the winners, so a collated batch stays grouped by item,
 * and equal xyz in two items never merge.  out_coords: int32 [n,4]; out_src: int32 [n], out_src[r] = the
 * input row that produced output row r; *out_count (device int64): the number of output rows, or
 * PCC_COUNT_ERR_RANGE when a result is not finite or lies beyond PCC_COORD_LIMIT or a batch index is not
 * in 0 .. nbatch-1 (such a value is never converted to an integer).  scratch: int32
 * [pcc_scan_scratch_elems(n)].  On return (keys, vals, cap) is the hash table of the OUTPUT set with
 * tensor stride 1, as for pcc_stride_map (cap >= pcc_hash_capacity(n)).
 * The reference removes NO duplicates (its first_occurrence_indices is the inverse map again, so it
 * returns N rows gathered from the first U); this is what its docstring says it does. */
int pcc_augment_rotate(const int32_t* coords, int64_t n, const float* rot, int32_t nbatch, float half,
                       uint64_t* keys, int32_t* vals, int64_t cap, int32_t* scratch, int32_t* out_coords,
                       int32_t* out_src, int64_t* out_count, void* stream);

/* ColorJitter (data/transform.py:107-130: torchvision.transforms.ColorJitter on float colours in [0,1]),
 * per batch item.  rgb, out: float32 [n,3]; offsets: DEVICE int64 [nbatch+1], item i owns rows
 * offsets[i] .. offsets[i+1]-1 (contiguous, ascending; an empty item is legal); params: float32 [nbatch,4]
 * = (brightness, contrast, saturation, hue) factors; order: int32 [nbatch,4], the order in which the four
 * operations (0 brightness, 1 contrast, 2 saturation, 3 hue) are applied to the item.
 *     gray(c) = 0.2989 r + 0.587 g + 0.114 b;     blend(a, b, f) = clamp(f a + (1 - f) b, 0, 1)
 *     brightness: blend(c, 0, f);   saturation: blend(c, gray(c), f)
 *     contrast:   blend(c, m, f), m = the mean of gray over the item's points at that stage of the chain
 *     hue:        RGB -> HSV (v = max, cr = max - min, s = cr / max or 0; rc, gc, bc = (max - r, g, b) / cr;
 *                 h6 = bc - gc | 2 + rc - bc | 4 + gc - rc by the channel of the maximum; h = fmod(h6 / 6 + 1, 1)),
 *                 h <- h + f wrapped into [0, 1), HSV -> RGB (i = floor(6h), t = 6h - i, p = clamp(v (1 - s)),
 *                 q = clamp(v (1 - t s)), u = clamp(v (1 - (1 - t) s)), sectors (v,u,p) (q,v,p) (p,v,u) (p,q,v) (u,p,v) (v,p,q))
 * The mean is a fixed-shape float64 sum over chunks of pcc_color_jitter_chunk() points counted from the
 * item's first row (no float atomics): results are bitwise equal from run to run, and an item gives the
 * same bytes alone and inside a batch.  Three launches whatever nbatch is.  scratch: 8-byte aligned,
 * pcc_color_jitter_scratch_bytes(n, nbatch) bytes. */
int32_t pcc_color_jitter_chunk(void);
int64_t pcc_color_jitter_scratch_bytes(int64_t n, int32_t nbatch);
int pcc_color_jitter(const float* rgb, int64_t n, const int64_t* offsets, int32_t nbatch, const float* params,
                     const int32_t* order, float* out, void* scratch, int64_t scratch_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * Voxelisation: raw points onto a voxel grid, with exact per-voxel attribute sums (the data front-end:
 * float PLYs, scans whose points collide on the grid, re-quantisation to fewer bits; the reference
 * down-samples its "QA" sequences through open3d's voxel_down_sample, data/utils/RawLoader.py:48-57).
 * xyz: float32 [n,3]; batch: int32 [n] or NULL (every point in item 0); attr: float32 [n,c] or NULL when
 * c = 0 (c = 0 .. 16).
 *   Cell.   Per axis g = (p - origin) / voxel, then floorf(g) (rounding 0) or rintf(g) (rounding 1, ties to
 *           even).  Every operation is rounded separately in fp32 and the division is a true, correctly
 *           rounded division, never a multiplication by a reciprocal: numpy's float32
 *           np.floor((p - o) / v) reproduces it bit for bit.  The grid is anchored at `origin`.
 *   Range.  A g that is not finite or lies beyond PCC_COORD_LIMIT is never converted to an integer.  Such a
 *           point, a batch index outside 0 .. nbatch-1, or an attribute that is not finite or has |a| > 1
 *           makes *out_count = PCC_COUNT_ERR_RANGE (the outputs are then unspecified).  voxel <= 0, not
 *           finite or NaN, a non-finite origin, c outside 0 .. 16, rounding other than 0 / 1, nbatch outside
 *           1 .. PCC_BATCH_LIMIT + 1, a capacity that is no power of two or below 2 n (pcc_hash_capacity(n) is one that fits), and
 *           null pointers are PCC_ERR_ARG, raised on the host before any launch.
 *   Order.  Output row r is the r-th distinct (batch, cell) in input order: out_coords int32 [n,4] (room for n
 *           rows, *out_count used), out_first[r] = the lowest input row that falls in it, out_row[i] = the
 *           output row of point i.  Equal cells of two batch items never merge.  On return (keys, vals, cap)
 *           is the hash table of the OUTPUT set with tensor stride 1, as after pcc_augment_rotate.
 *   Sums.   Each attribute is converted once to Q32 fixed point, q = llrint((double)a * 4294967296.0) (ties
 *           to even): a = k/255 is represented exactly, only values below 2^-8 round at all, by at most
 *           2^-33.  out_sum int64 [n,c]: per voxel and channel the int64 sum of the q; out_npts int32 [n]:
 *           the number of points.  With |a| <= 1 and n < 2^31 no sum overflows.  Integer addition commutes:
 *           any schedule gives the same bytes (integer atomics, no float atomics).
 *   Mean.   Left to the caller: float32(float64(sum) / float64(npts) / 2^32).
 * The call initialises everything it accumulates into (rows 0 .. count-1 of out_npts / out_sum): buffers
 * may be handed over uninitialised; rows behind the count are not written.  scratch: int32
 * [pcc_scan_scratch_elems(n)].  Eight launches (clear, claim, flag, three scan kernels, finalize,
 * accumulate); n = 0 is valid (*out_count = 0). */
int pcc_voxelize(const float* xyz, const int32_t* batch, int64_t n, int32_t nbatch, const float* attr, int32_t c,
                 float origin_x, float origin_y, float origin_z, float voxel, int32_t rounding, uint64_t* keys,
                 int32_t* vals, int64_t cap, int32_t* scratch, int32_t* out_coords, int32_t* out_first,
                 int32_t* out_npts, int64_t* out_sum, int32_t* out_row, int64_t* out_count, void* stream);

/* ---------------------------------------------------------------------------------------
 * Position scaling: lossy geometry by a rational scale, with the colours moved onto the quantised geometry
 * ("recolouring") — what a conventional coder does at positionQuantizationScale < 1 (the reference's G-PCC
 * operating points, plot.py:34 and evaluate_view_dep.py:95: scales 0.125, 0.25, 0.5, 0.75).
 *   Scale.  s = num / den with integers 1 <= num <= den <= 255.  Per axis, in integers, with FLOOR division
 *           (also for negative coordinates):
 *               cell(p) = floor((2 p num + den) / (2 den))      p s rounded to nearest, halves up
 *               pos(c)  = floor((2 c den + num) / (2 num))      c / s rounded to nearest, halves up
 *           pos is strictly increasing (cells are at least one voxel apart), so distinct cells have distinct
 *           positions and the lexicographic order of positions is that of cells; cell(pos(c)) = c.
 *   Range.  A source coordinate beyond PCC_COORD_LIMIT, or a position that would fall beyond it, is an error
 *           the caller raises on the host from the cloud's extent before a kernel runs (pos is monotone: the
 *           extremes decide).  On the device a point with a coordinate beyond the limit, a batch index beyond
 *           PCC_BATCH_LIMIT or an attribute that is not finite or has |a| > 1 makes pcc_scaled_cells report
 *           *out_count = PCC_COUNT_ERR_RANGE (the outputs are then unspecified), as in pcc_voxelize.
 *           num / den outside the range above, c outside 0 .. 16, a capacity that is no power of two or below
 *           2 n, and null pointers are PCC_ERR_ARG, raised on the host before any launch.  n = 0 is valid.
 *
 * pcc_scaled_cells: coords int32 [n,4] (batch, x, y, z), attr float32 [n,c] or NULL when c = 0.  Outputs as
 *   pcc_voxelize gives them: out_coords [n,4] = the distinct (batch, cell) in order of first appearance
 *   (*out_count rows), out_first, out_npts, out_row, and out_sum int64 [n,c] = the exact Q32 sums of each
 *   cell's OWN points (q = llrint((double)a * 4294967296.0)); on return (keys, vals, cap) is the hash table
 *   of the cell set with tensor stride 1.  scratch: int32 [pcc_scan_scratch_elems(n)].  Eight launches.
 *
 * pcc_scaled_transfer: the same points and attributes, the table of their cell set (m rows), num, den.
 *   Per point: out_nearest[i] = the cell row whose position pos(cell) is nearest to the point, out_d2[i]
 *   (int64) = the squared distance in original voxels.  Per cell row: out_npts[r] = how many points chose
 *   it, out_sum[r, ch] = the Q32 sum of their attributes; the call clears rows 0 .. m-1 of both first.
 *   Ties.   Equidistant candidates resolve to the smallest (x, y, z), the rule of pcc_nn_search.  A cell of
 *           another batch item is never a candidate.
 *   Walk.   One thread per point walks shells k = 0, 1, 2 ... of Chebyshev radius k in the CELL domain
 *           around cell(p) and measures true distances to pos(c).  Every cell of shell k differs from
 *           cell(p) by exactly k along some axis a, and pos is monotone with pos(cell(p) - 1) < p <
 *           pos(cell(p) + 1), so its distance^2 is at least
 *               L(k) = min over a of min((pos(c0_a + k) - p_a)^2, (p_a - pos(c0_a - k))^2),
 *           which does not decrease with k.  The walk stops before shell k once best < L(k); at best == L(k)
 *           a tie may still be in shell k, so it is scanned.  Shell 0 holds the point's own cell, which is
 *           in the set: the walk always ends, with no maximum radius and no retry on the host.  (A point
 *           whose own cell is NOT in the table — a foreign table — or with a coordinate out of range gets
 *           out_nearest = out_d2 = -1 and adds nothing.)
 *   Sums.   Integer atomics only, behind the in-wave fold of equal rows the voxelisation uses: the outputs
 *           are bitwise reproducible under any schedule.  The attributes are not range-checked again.
 *   Two launches (clear, walk).
 * ------------------------------------------------------------------------------------- */
int pcc_scaled_cells(const int32_t* coords, int64_t n, const float* attr, int32_t c, int32_t num, int32_t den,
                     uint64_t* keys, int32_t* vals, int64_t cap, int32_t* scratch, int32_t* out_coords,
                     int32_t* out_first, int32_t* out_npts, int64_t* out_sum, int32_t* out_row, int64_t* out_count,
                     void* stream);
int pcc_scaled_transfer(const int32_t* coords, int64_t n, const float* attr, int32_t c, int32_t num, int32_t den,
                        const uint64_t* keys, const int32_t* vals, int64_t cap, int64_t m, int32_t* out_nearest,
                        int64_t* out_d2, int32_t* out_npts, int64_t* out_sum, void* stream);

/* Kernel map (ME kernel_map, cached per coordinate manager): for every output row j and
 * kernel offset k, nbr[j*K + k] = input row at c_out + sign * off_k * step, or -1.
 * sign = +1 for (strided) convolution with step = input tensor stride; sign = -1 for
 * transposed / generative convolution with step = input stride / 2.
 * row_mask[j] (uint32) has bit k set iff output row j has a neighbour at offset k.
 * *pair_count (device int64, may be NULL) receives the number of (output row, offset) pairs
 * with a neighbour = the "pairs" of the algorithmic FLOP count 2 * pairs * C_in * C_out. */
int pcc_kernel_map(const int32_t* out_coords, int64_t n_out, const uint64_t* in_keys,
                   const int32_t* in_vals, int64_t in_cap, int32_t ksize, int32_t step,
                   int32_t sign, int32_t* nbr, uint32_t* row_mask, int64_t* pair_count,
                   void* stream);

/* The pair count of a kernel map from its row masks alone (sum of popcounts) — for callers that passed
 * pair_count = NULL to pcc_kernel_map and want the figure later (FLOP accounting of a benchmark: the codec itself
 * never reads it, so the product path does not compute it per map). */
int pcc_pair_count(const uint32_t* row_mask, int64_t n_out, int64_t* pair_count, void* stream);

/* Execution order for the MFMA convolution.  Output rows are sorted by
 * (spatial block of 2^block_log2 voxels per axis, neighbour mask); block_log2 < 0 sorts by
 * mask alone.  Rows with the same neighbour pattern become adjacent, so a 32-row MFMA tile
 * multiplies (almost) no all-zero neighbour rows.  Results do not depend on the order.
 *   order[p]        = output row executed at position p
 *   group_mask32[g] = OR of row_mask over positions 32g .. 32g+31
 * The neighbour table itself stays in output-row order: the convolution kernels read row order[p] of it.
 * scratch_bytes from pcc_order_scratch_bytes(n). */
int64_t pcc_order_scratch_bytes(int64_t n);
int pcc_order_rows_by_mask(const uint32_t* row_mask, const int32_t* coords, int64_t n,
                           int32_t block_log2, int32_t tensor_stride, int32_t* order, uint32_t* group_mask32,
                           void* scratch, int64_t scratch_bytes, void* stream);
/* nbr_sorted[p, :] = nbr[order[p], :] — the permuted copy of a table for the weight-gradient kernels of the training
 * path, which index their table by execution position (pcc_conv_wgrad*). */
int pcc_permute_map_rows(const int32_t* nbr, const int32_t* order, int64_t n, int32_t K, int32_t* nbr_sorted, void* stream);

/* pcc_kernel_map + pcc_order_rows_by_mask (mask order over the whole map: block_log2 < 0) in ONE launch for maps of at
 * most pcc_small_map_max() output rows (256; 0 when PCC_SMALL_MAP=0): a single 1024-thread workgroup probes, counts, builds
 * the keys and sorts — three launches otherwise (six and a memset above 16,384 rows), each a few microseconds of work
 * behind its dispatch; from ~300 rows on the probes are too much work for one CU.
 * Outputs as those two calls write them, bit for bit (nbr [n_out, K], row_mask, order, group_mask32);
 * scratch_bytes from pcc_order_scratch_bytes(n_out). */
int64_t pcc_small_map_max(void);
/* One-workgroup forms of the small per-map chains, as a bit mask: 1 = execution order (maps of at most 16,384 rows: counts, keys and
 * sort in one launch), 2 = top-k (one batch item, at most 32,768 rows), 4 = coordinate sets (at most 8,192 candidates).  All on
 * by default (PCC_ORDER_SMALL=0 / PCC_TOPK_SMALL=0 / PCC_UNIQUE_SMALL=0 switch one off at start-up); sets the mask and returns
 * the previous one, a negative argument only reads it.  Outputs do not depend on it. */
int32_t pcc_small_paths(int32_t mask);
int pcc_small_kernel_map(const int32_t* out_coords, int64_t n_out, const uint64_t* in_keys, const int32_t* in_vals, int64_t in_cap,
                         int32_t ksize, int32_t step, int32_t sign, int32_t* nbr, uint32_t* row_mask, int32_t* order,
                         uint32_t* group_mask32, void* scratch, int64_t scratch_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * Sparse convolution forward (ME.MinkowskiConvolution / *ConvolutionTranspose forward,
 * 100+ instances: model/transforms.py:35-57,168-234; model/blocks.py:17-24,86-97,194-220;
 * model/entropy_models.py:273-305) with the pointwise ops that follow it fused:
 *   v = bias + sum_k in[nbr(j,k)] @ W[k]                 (k ascending, fixed order)
 *   if film:     v = v * film[j, c] + film[j, cout + c]   (ScaledBlock, blocks.py:37-40)
 *   v = act(v)                                            (MinkowskiReLU / LeakyReLU)
 *   if residual: v += residual[j, c]                      (blocks.py:49-52)
 * W is the ME kernel tensor [K, cin, cout] (fp32).  For cin % 32 == 0 the MFMA path is used
 * and needs `w_packed` from pcc_conv_pack_weights; otherwise (cin in {1,2,3,4,6,8,12,16,24}) the
 * thin path reads `w` directly.  nbr == NULL means kernel_size 1 (identity map, K = 1).
 * MFMA path: if `order` != NULL, position p computes output row order[p] and `group_mask32` holds the
 * masks from pcc_order_rows_by_mask; with order == NULL rows run in natural order (group_mask32 may
 * then be NULL = every offset executed).
 * nbr / film / residual / fout are always indexed by the output row, never by the position.
 * MFMA path (also pcc_conv_fwd_bf16, pcc_conv_wgrad*): the gathered tensors (fin, dy) and
 * w_packed must be 16-byte aligned — rows move by 16-byte LDS-DMA loads; PCC_ERR_ARG otherwise.
 * ------------------------------------------------------------------------------------- */
int64_t pcc_conv_packed_elems(int32_t K, int32_t cin, int32_t cout);
int pcc_conv_pack_weights(const float* w, int32_t K, int32_t cin, int32_t cout, float* w_packed,
                          void* stream);
int pcc_conv_fwd(const float* fin, int64_t n_in, int32_t cin, const float* w, const float* w_packed,
                 const float* bias, const int32_t* nbr, const int32_t* order,
                 const uint32_t* group_mask32, int32_t K, float* fout, int64_t n_out, int32_t cout,
                 int32_t act, const float* film, const float* residual, void* stream);

/* Small launches of pcc_conv_fwd (map convolutions, cin % 32 == 0, whose 32 x 32 output tiles number at most
 * `workgroups`, twice that for outputs narrower than 128 columns) run on conv_small_kernel: one 16 x 16 MFMA block per wave,
 * loader waves running the LDS-DMAs ahead — the time of such a launch is one workgroup's serial MFMA chain, which this makes
 * four times shorter (128 -> 128 on 1,136 rows: 27 us against 66).  Results are bit-identical.  Sets the threshold (default
 * 640, or PCC_CONV_SMALL_MAX; 0 = never) and returns the previous one; a negative argument only reads it. */
int64_t pcc_conv_small_max(int64_t workgroups);

/* The kernel a forward launch of `mode` (0 = pcc_conv_fwd, 1 = pcc_conv_fwd_bf16, 2 = pcc_conv_fwd_x3) runs on this shape,
 * spelled as the profiler prints it (bf16 / x3 names carry a "[bf16]" / "[x3]" tag after the kernel's name), written to
 * `buf` (`len` bytes; buf == NULL only asks whether the mode runs the shape).  Host only, launches nothing.
 * PCC_ERR_UNSUPPORTED when that mode cannot run the shape. */
int pcc_conv_kernel_name(int32_t mode, int64_t n_in, int32_t cin, int32_t cout, int64_t n_out, int32_t K, int32_t has_nbr,
                         char* buf, int32_t len);

/* bf16-input variant of pcc_conv_fwd (training / BASELINE config 5): features and packed weights are bf16
 * (fin [n_in, cin] bf16, cin a multiple of 64; pcc_conv_pack_weights_bf16: [K, cin/8, cout^32, 8]), products
 * accumulate in fp32 on v_mfma_f32_32x32x16_bf16, bias / FiLM / activation / residual and the output are fp32.
 * Same tiling, row order, offset skipping and accumulation order as the fp32 kernel; half the gather bytes
 * and 1/8 of the MFMA time per channel.  NOT used by compress / decompress (fp32 parity budget). */
int64_t pcc_conv_packed_elems_bf16(int32_t K, int32_t cin, int32_t cout);
int pcc_conv_pack_weights_bf16(const float* w, int32_t K, int32_t cin, int32_t cout, uint16_t* w_packed, void* stream);
int pcc_conv_fwd_bf16(const uint16_t* fin, int64_t n_in, int32_t cin, const uint16_t* w_packed, const float* bias,
                      const int32_t* nbr, const int32_t* order, const uint32_t* group_mask32, int32_t K, float* fout,
                      int64_t n_out, int32_t cout, int32_t act, const float* film, const float* residual, void* stream);

/* Training-path epilogue of a convolution as its own operator (the inference path fuses it into pcc_conv_fwd):
 *   forward   out = act(film ? c * beta + gamma : c) + (residual ? residual : 0)     (blocks.py:37-40,49-52)
 *   backward  du = dout * act'(u);  dc = film ? du * beta : du;  dfilm = [du * c | du]   (d residual = dout)
 * c / out / dout / dc [n, channels], film / dfilm [n, 2 * channels] (beta | gamma); channels % 4 == 0, 16-byte aligned.
 * Same operation order as the torch ops they replace (mul, add, act, add): identical values and gradients. */
int pcc_epilogue_fwd(const float* c, const float* film, const float* residual, int64_t n, int32_t channels, int32_t act,
                     float* out, void* stream);
int pcc_epilogue_bwd(const float* dout, const float* c, const float* film, int64_t n, int32_t channels, int32_t act,
                     float* dc, float* dfilm, void* stream);

/* dY of a convolution read once on the training path (autograd.py, SparseConvFn.backward): out_bf16 (may be NULL) = the
 * bf16 copy the bf16 weight-gradient / backward-data kernels gather (round to nearest even, torch's conversion), colsum
 * (may be NULL) = the column sums = the bias gradient (ME differentiates `out + bias`, reference blocks.py convolutions
 * with bias=True).  Deterministic two-stage reduction; scratch: pcc_cast_colsum_scratch_elems(channels) floats.
 * channels % 4 == 0, <= 1024; x 16-byte aligned. */
int64_t pcc_cast_colsum_scratch_elems(int32_t channels);
int pcc_cast_colsum(const float* x, int64_t n, int32_t channels, uint16_t* out_bf16, float* colsum, float* scratch,
                    int64_t scratch_elems, void* stream);

/* Split-bf16 arithmetic on fp32 data (opt-in; the default convolution multiplies in fp32): every fp32 operand is
 * the exact sum of three bf16 numbers; the weights are pre-split into three planes (pcc_conv_pack_weights_x3,
 * pcc_conv_packed_elems_x3 bf16 elements), the gathered fp32 rows are split in registers, and the six products
 * whose weight is at least 2^-16 of the leading one run on v_mfma_f32_32x32x16_bf16 with fp32 accumulation in a
 * fixed order.  Same semantics, epilogue and determinism guarantees as pcc_conv_fwd; results differ from it by
 * the size of an fp32 rounding per product (dropped terms < 3 x 2^-24 |x||w|).  cin % 32 == 0, cin <= 256, output
 * width (rounded up to 32) a multiple of 64; encoder and decoder must use the same mode. */
int64_t pcc_conv_packed_elems_x3(int32_t K, int32_t cin, int32_t cout);
int pcc_conv_pack_weights_x3(const float* w, int32_t K, int32_t cin, int32_t cout, uint16_t* w_packed, void* stream);
int pcc_conv_fwd_x3(const float* fin, int64_t n_in, int32_t cin, const uint16_t* w_packed, const float* bias,
                    const int32_t* nbr, const int32_t* order, const uint32_t* group_mask32, int32_t K, float* fout,
                    int64_t n_out, int32_t cout, int32_t act, const float* film, const float* residual, void* stream);

/* Thin inputs, wide outputs (cin <= 8, cout % 32 == 0: the first layers of the q-map heads and of g_a) on the matrix cores:
 * out[j, :] = the K * cin inputs of output row j's neighbourhood (zeros for absent neighbours), zero-padded to k2 (a multiple
 * of 32) columns, stored in the order pcc_conv_fwd's MFMA loop contracts channels — physical column 8 g + s holds logical
 * column 8 g + 2 (s & 3) + (s >> 2), logical = k * cin + ci.  Followed by a kernel_size-1 pcc_conv_fwd over `out` with the
 * weights re-laid-out the same way ([1, k2, cout]: row 8 g + [0,4,1,5,2,6,3,7][t] = W[k, ci, :] of logical 8 g + t), the sum
 * per output element runs over (k, ci) ascending like the scalar thin kernel's: identical bits, the fp32 MFMA being the
 * same fused multiply-add chain as v_fma_f32. */
int pcc_im2col_thin(const float* fin, int32_t cin, const int32_t* nbr, int64_t n_out, int32_t K, float* out, int32_t k2,
                    void* stream);

/* Narrow-head convolution, second half (cout <= 4 on wide inputs: the occupancy logit of
 * model/blocks.py:94-98,142 and the q-map heads).  The caller first computes
 * scores[i, k*cout + c] = in[i] . W[k][:, c] for every INPUT row with one kernel_size-1 call of
 * pcc_conv_fwd on the re-laid-out kernel [cin, K*cout]; this call adds, per output row, the
 * <= K scalars its neighbours contribute: out[j,c] = act(bias[c] + sum_k scores[nbr(j,k), k*cout+c]).
 * `nbr` is the natural-order table of pcc_kernel_map; `ld` = row stride of scores in floats. */
int pcc_gather_sum_fwd(const float* scores, int32_t ld, const int32_t* nbr, int32_t K, int32_t cout,
                       const float* bias, float* out, int64_t n_out, int32_t act, void* stream);

/* ---------------------------------------------------------------------------------------
 * Row movement: lookup-gather, pruning.
 * ------------------------------------------------------------------------------------- */
/* out[i,:] (+)= idx[i] >= 0 ? src[idx[i],:] : 0   (features_at_coordinates after
 * pcc_hash_lookup; accumulate != 0 adds into out: model/transforms.py:96,262). */
int pcc_gather_rows(const float* src, int32_t c, const int32_t* idx, int64_t n, float* out,
                    int32_t accumulate, void* stream);

/* out[idx[i],:] = src[i,:] for idx[i] >= 0 (re-indexing a tensor onto another map). */
int pcc_scatter_rows(const float* src, int32_t c, const int32_t* idx, int64_t n, float* out,
                     void* stream);
/* out[idx[i],:] += src[i,:] for idx[i] >= 0: the backward of pcc_gather_rows (training path; the
 * reference gets it from torch's indexing autograd behind features_at_coordinates, loss.py:103-107). */
int pcc_scatter_add_rows(const float* src, int32_t c, const int32_t* idx, int64_t n, float* out,
                         void* stream);

/* ME.MinkowskiPruning (model/blocks.py:90,126): order-preserving compaction of the rows
 * with mask != 0.  Either of feats/out_feats and coords/out_coords may be NULL.
 * new_index[i] (optional) = output row of input row i or -1.  *out_count: device int64. */
int pcc_compact_rows(const uint8_t* mask, int64_t n, const int32_t* coords, int32_t* out_coords,
                     const float* feats, int32_t c, float* out_feats, int32_t* new_index,
                     int32_t* scratch, int64_t* out_count, void* stream);

/* ---------------------------------------------------------------------------------------
 * Per-batch top-k on one logit per row (GenerativeUpBlock._topk_prediction,
 * model/blocks.py:130-150, torch.topk).  Row i belongs to batch coords[i*4]; batch b keeps
 * its k[b] largest logits (logits[i*ld]); exact ties are broken by ascending voxel key.
 * NaN sorts above +inf (torch.topk); -0 equals +0.  Batch b keeps max(0, min(k[b], rows of b)) rows; rows whose batch index
 * is outside [0, nbatch) are never selected and never counted.
 * Precondition of nbatch == 1: EVERY row belongs to batch 0.  The passes over the logit bytes then do not read the
 * coordinates: a row with another index would be counted there and never selected, so fewer than k rows would come out.
 * state: >= pcc_topk_state_elems(nbatch) int32 elements (per item the selection's words and a
 * 256-bin histogram; for one item also the 256 x 256 per-workgroup bins of the logit passes).
 * ------------------------------------------------------------------------------------- */
int64_t pcc_topk_state_elems(int32_t nbatch);
int pcc_topk_mask(const float* logits, int32_t ld, const int32_t* coords, int64_t n, int32_t nbatch,
                  const int32_t* k, uint8_t* mask, int32_t* state, void* stream);

/* rows-per-batch histogram (AnalysisTransform.count_per_batch, model/transforms.py:65-71). */
int pcc_count_per_batch(const int32_t* coords, int64_t n, int32_t nbatch, int32_t* counts, void* stream);

/* Canonical (b,x,y,z)-lexicographic order (utils.sort_tensor / sort_points,
 * utils.py:155-204): perm[r] = input row that comes r-th.  scratch_bytes from the query. */
int64_t pcc_sort_scratch_bytes(int64_t n);
int pcc_sort_coords(const int32_t* coords, int64_t n, int32_t* perm, void* scratch,
                    int64_t scratch_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * Convolution backward (training path; the reference gets it from MinkowskiEngine's autograd
 * functions behind every ME.Minkowski*Convolution*, train.py:194-206).
 *   dX = pcc_conv_fwd over the TRANSPOSED map with transposed weights W^T[k] = W[k]^T:
 *        pcc_kernel_map_transpose gives nbr_t[i, k] = output row j with nbr[j, k] == i (or -1) and
 *        the per-input-row offset masks (feed them to pcc_order_rows_by_mask like a forward map).
 *   dW[k] = sum over the pairs of offset k of X[i]^T dY[j]: pcc_conv_wgrad (nbr / order / group masks
 *        of the FORWARD map in execution order; order == NULL: natural order).  fp32 MFMA for
 *        cin, cout multiples of 32, a scalar kernel for thin shapes (cin * cout <= 4096).  The
 *        reduction order is fixed (bitwise reproducible).  scratch: pcc_conv_wgrad_scratch_elems floats.
 *   db = column sums of dY (caller).
 * ------------------------------------------------------------------------------------- */
int pcc_kernel_map_transpose(const int32_t* nbr, int64_t n_out, int32_t K, int64_t n_in, int32_t* nbr_t,
                             uint32_t* row_mask_t, void* stream);
int64_t pcc_conv_wgrad_scratch_elems(int32_t K, int32_t cin, int32_t cout);
int pcc_conv_wgrad(const float* fin, int64_t n_in, int32_t cin, const float* dy, int64_t n_out, int32_t cout,
                   const int32_t* nbr, const int32_t* order, const uint32_t* group_mask32, int32_t K, float* dw,
                   float* scratch, int64_t scratch_elems, void* stream);
/* The kernel a weight-gradient launch runs on this shape (bf16 = 0: pcc_conv_wgrad, 1: pcc_conv_wgrad_bf16), spelled as the
 * profiler prints it, e.g. "conv_wgrad_slice_kernel<5, 2>", written to `buf` (`len` bytes; buf == NULL leaves it out);
 * *split = row-group splits of the launch, *partials = images [K][cin][cout] its second stage adds (either may be NULL).
 * n_out <= 0 gives an empty name and zeros: the launch only zero-fills dw.  Host only, launches nothing.  A shape the launch
 * refuses gives the launch's error code. */
int pcc_conv_wgrad_kernel_name(int32_t bf16, int32_t K, int32_t cin, int32_t cout, int64_t n_out, char* buf, int32_t len,
                               int32_t* split, int32_t* partials);
/* bf16 operands (fin, dy bf16; cin, cout multiples of 64), fp32 accumulation and result; same scratch size. */
int pcc_conv_wgrad_bf16(const uint16_t* fin, int64_t n_in, int32_t cin, const uint16_t* dy, int64_t n_out, int32_t cout,
                        const int32_t* nbr, const int32_t* order, const uint32_t* group_mask32, int32_t K, float* dw,
                        float* scratch, int64_t scratch_elems, void* stream);

/* ---------------------------------------------------------------------------------------
 * Channelwise (depthwise) window convolution on ONE coordinate set, stride 1, and its adjoint
 * (ME.MinkowskiChannelwiseConvolution: the window sums of ColorSSIM, loss.py:204-206, 391-453).
 *   y[i, ch] = sum_k w[k', ch] * x[row(coords[i] + offset(k) * tensor_stride), ch]
 * over the offsets whose voxel exists in the set (absent neighbours, and neighbours whose coordinate
 * leaves the key range, contribute nothing; the batch index is part of the key, so a window never
 * crosses batch items).  k = (dx+h) + ksize (dy+h) + ksize^2 (dz+h), h = ksize / 2 (x fastest);
 * k' = k for flip = 0 and ksize^3 - 1 - k for flip = 1.  Input and output set are the same, so
 * flip = 1 with the same window is exactly the adjoint: backward-data is this call on dY.
 * x, y [n, c] fp32 (c = 1 .. 32); coords [n, 4] and (keys, vals, cap, tensor_stride) the set and its
 * table (vals = row of x); w [ksize^3, w_channels] with w_channels = 1 (one window for every channel)
 * or c; ksize odd, 1 .. 11.  Anything else is refused before any launch (PCC_ERR_UNSUPPORTED for a
 * kernel size or channel count outside the range, else PCC_ERR_ARG); n == 0 launches nothing.
 * The neighbour table is never stored: one kernel probes and accumulates.  Deterministic, no atomics:
 * an element starts at +0 and adds its present neighbours' products one by one in ascending
 * (dz+h) + ksize (dy+h) + ksize^2 (dx+h) — z fastest, for either flip — each product rounded to fp32
 * before the add (separate multiply and add, no fused multiply-add).
 * ------------------------------------------------------------------------------------- */
int pcc_chconv(const float* x, int64_t n, int32_t c, const int32_t* coords, const uint64_t* keys, const int32_t* vals,
               int64_t cap, int32_t tensor_stride, int32_t ksize, const float* w, int32_t w_channels, int32_t flip,
               float* y, void* stream);

/* ---------------------------------------------------------------------------------------
 * Latent-coordinate side channel of file mode.  Replaces ColorModel.gpcc_encode / gpcc_decode
 * (model/model.py:318-395), which shell out to the external MPEG G-PCC binary `tmc3`; this is the
 * build's own lossless octree ("PCO1", NOT G-PCC compatible; container in octree.py).
 *
 * pcc_octree_occupancy: coords [n,4] (batch ignored), grid = (c - origin) / stride must lie in
 *   [0, 2^depth)^3.  Child index per level = (xbit << 2) | (ybit << 1) | zbit.  Level L
 *   (0 = root .. depth-1) receives one occupancy byte per occupied node, ascending Morton order,
 *   at occupancy[L * n ...]; level_counts (device, depth + 2 ints) = nodes per level, then the
 *   number of distinct leaves (== n unless the input holds duplicates), then the number of
 *   inputs outside the grid / off the stride lattice (must be 0).  origin: 3 host ints.
 * pcc_octree_expand: the inverse.  occupancy = the levels back to back (device), level_counts
 *   = depth host int64; writes coords_out [n_points,4] = (batch, x, y, z) in ascending Morton
 *   order.  The caller has already checked that the popcounts of level L sum to the size of
 *   level L+1 (n_points for the last); a stream that lies cannot write out of bounds.
 * ------------------------------------------------------------------------------------- */
int64_t pcc_octree_scratch_bytes(int64_t n);
int pcc_octree_occupancy(const int32_t* coords, int64_t n, int32_t stride, const int32_t* origin,
                         int32_t depth, uint8_t* occupancy, int32_t* level_counts, void* scratch,
                         int64_t scratch_bytes, void* stream);
int pcc_octree_expand(const uint8_t* occupancy, const int64_t* level_counts, int32_t depth,
                      int32_t stride, const int32_t* origin, int32_t batch, int64_t n_points,
                      int32_t* coords_out, void* scratch, int64_t scratch_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * Neighbour contexts of the octree coder (the opt-in stream "PCO2"; container and model in
 * octree.py, DESIGN.md "Octree contexts (PCO2)").  The pattern of a node at level L is 6 bits,
 * bit 0 +x, 1 -x, 2 +y, 3 -y, 4 +z, 5 -z, set when that face neighbour is an occupied node of
 * level L; a neighbour outside [0, 2^L)^3 is absent.  Bit j of a node's occupancy byte is a
 * binary symbol with context pattern * 8 + j (512 contexts).
 *
 * pcc_octree_context_levels: pcc_octree_occupancy (same arguments, same occupancy and
 *   level_counts), and in the same layout patterns[L * n ...] = one pattern byte per node, and
 *   hists [depth, 512, 2] uint32 (device; zeroed here) = per level the number of (context, bit)
 *   pairs.  Integer atomics only: the histograms do not depend on the order of execution.
 * pcc_octree_patterns: nodes = the n ascending 3*level-bit Morton keys of one level (device)
 *   -> patterns [n].
 * pcc_octree_expand_level: one step of pcc_octree_expand.  nodes [n] and their occupancy bytes
 *   [n] (device) -> next [n_next], the keys (node << 3) | child of the next level, ascending.
 *   The caller has checked that no byte is 0 and that the popcounts sum to n_next; children
 *   past n_next are dropped, never written.  scratch: pcc_octree_scratch_bytes(n).
 * pcc_octree_keys_to_coords: leaf keys [n] (device) -> coords_out [n,4] = (batch, x, y, z).
 * ------------------------------------------------------------------------------------- */
int pcc_octree_context_levels(const int32_t* coords, int64_t n, int32_t stride, const int32_t* origin,
                              int32_t depth, uint8_t* occupancy, uint8_t* patterns, uint32_t* hists,
                              int32_t* level_counts, void* scratch, int64_t scratch_bytes, void* stream);
int pcc_octree_patterns(const uint64_t* nodes, int64_t n, int32_t level, uint8_t* patterns, void* stream);
int pcc_octree_expand_level(const uint64_t* nodes, const uint8_t* occupancy, int64_t n, int64_t n_next,
                            uint64_t* next, void* scratch, int64_t scratch_bytes, void* stream);
int pcc_octree_keys_to_coords(const uint64_t* keys, int64_t n, int32_t stride, const int32_t* origin,
                              int32_t batch, int32_t* coords_out, void* stream);

/* ---------------------------------------------------------------------------------------
 * Quality metrics: nearest-neighbour association on integer grids.  Replaces the open3d KD-tree
 * queries of PointCloudMetric (metrics/metric.py:36-43).  For every query row (b,x,y,z) finds the
 * nearest target voxel through the target's hash table (pcc_hash_build): nn_idx = target row,
 * nn_d2 = squared Euclidean distance (sum over axes, NOT the reference's per-axis mean);
 * equidistant candidates resolve to the smallest (x,y,z); tie_count / tie_rgb (optional) = number
 * of equidistant nearest voxels and the sum of their colours (target_rgb [n,3], f64 like the
 * reference's numpy arrays) for the reference's
 * tie-averaging mode (metric.py:121-146).  Queries whose neighbour is farther than max_radius
 * (Chebyshev shells searched: 0..max_radius) get nn_idx = nn_d2 = -1 and must be retried wider.
 * ------------------------------------------------------------------------------------- */
int pcc_nn_search(const int32_t* query, int64_t nq, const uint64_t* keys, const int32_t* vals, int64_t cap,
                  int32_t tensor_stride, const double* target_rgb, int32_t max_radius, int32_t* nn_idx, int64_t* nn_d2,
                  int32_t* tie_count, double* tie_rgb, void* stream);

/* ---------------------------------------------------------------------------------------
 * Surface normals of a voxelised cloud (point-to-plane / D2 PSNR, facing quality maps).  Replaces
 * open3d's estimate_normals (evaluate_view_dep.py:354-376).  coords [n,4] = (batch, x, y, z);
 * keys / vals / cap / tensor_stride: the hash table of the SAME cloud (pcc_hash_build).  The
 * neighbourhood of a point p is every occupied voxel q of its batch item with d = q - p and
 * d.d <= radius^2 (p included; radius 1..8).  count [n] (optional) = its size; moments [n,6]
 * (optional) = the upper triangle (xx, xy, xz, yy, yz, zz) of M = count * sum(d d^T) -
 * sum(d) sum(d)^T, exact integers.  normals [n,3] (f64) = the unit eigenvector of M's smallest
 * eigenvalue (cyclic Jacobi, fixed order and sweeps: bitwise reproducible), or (0,0,0) where
 * count < 3 or the neighbours are collinear (sum of M's principal 2 x 2 minors <= 0, in int64).
 * orient_mode 0: sign as computed; 1: n.orient >= 0; 2: n.(orient - p) >= 0 (orient = a camera
 * position).  orient: 3 HOST doubles (may be NULL in mode 0).
 * ------------------------------------------------------------------------------------- */
int pcc_estimate_normals(const int32_t* coords, int64_t n, const uint64_t* keys, const int32_t* vals, int64_t cap,
                         int32_t tensor_stride, int32_t radius, int32_t orient_mode, const double* orient,
                         double* normals, int32_t* count, int64_t* moments, void* stream);

/* ---------------------------------------------------------------------------------------
 * Perceptual metric "pcqm_voxel": PCQM's structure (Meynet, Nehme, Digne, Lavoue, QoMEX 2020) on a voxel
 * grid.  A stand-in for the external PCQM binary of the reference's sweep (utils.py:290-344); it does NOT
 * reproduce that binary's numbers (plain CIELAB instead of LAB2000HL, surface variation instead of a quadric's
 * mean curvature, nearest voxel instead of a projection onto a quadric).
 *
 * pcc_surface_variation: kappa [n] (f64) = l0 / (l0 + l1 + l2), l0 <= l1 <= l2 the eigenvalues of the moment
 * matrix M of pcc_estimate_normals over the radius-`radius` ball (1..8), by the same fixed-order Jacobi
 * (bitwise reproducible; an l0 below zero counts as 0); 0 where pcc_estimate_normals gives no normal.
 * coords / keys / vals / cap / tensor_stride: one cloud and its own table.
 *
 * pcc_pcqm_features: one logical work item per row p of the reference cloud R (coords_r [n_r,4] and its
 * table); D (coords_d [n_d,4] and its table) is the distorted cloud, nn [n_r] the row of p's nearest D voxel
 * p^.  attrs_r [n_r,5] / attrs_d [n_d,5] (f64): (L, c, a, b, kappa) per row.  w: h^2 + 1 device doubles, the
 * weight of a neighbour at squared distance d2 is w[d2] (h: 1..8).  constants: 4 HOST doubles (k_L, k_kappa,
 * c_chroma, c_hue).  N_R(p) = rows q of R with |q - p|^2 <= h^2, N_D(p^) likewise in D, centres included,
 * each ball walked once in ascending (dx, dy, dz).  Outputs (device f64, each may be NULL, not all three):
 *   stats [n_r,18]: sum of w over N_R, over N_D; the weighted means of L, c, a, b, kappa over N_R, then over
 *     N_D; then v_L, v^_L, s_L, v_kappa, v^_kappa, s_kappa: the weighted variances over N_R and N_D (clamped
 *     at 0) and the cross term s_x = sum_{q in N_R} w (x_R(q) - mean_R)(x_D(nn[q]) - mean_D) / sum w.
 *   features [n_r,8]: f1 = |mL - m^L| / (max + k_L), f2 = the same on sqrt(v_L), sqrt(v^_L),
 *     f3 = |S - s_L| / (S + k_L) with S = sqrt(v_L v^_L), f4 = 1 - 1 / (c_chroma (mc - m^c)^2 + 1),
 *     f5 = 1 - 1 / (c_hue dH + 1) with dH = max(0, (ma - m^a)^2 + (mb - m^b)^2 - (mc - m^c)^2), f6..f8 = f1..f3
 *     on kappa with k_kappa.  Identical clouds give exactly 0 everywhere.
 *   sums [8]: the sums of the features over all rows; needs scratch of pcc_pcqm_scratch_bytes(n_r) bytes (0
 *     for an n the call refuses): workgroups store partial sums in workgroup order, a second launch adds them
 *     in ascending order.  No float atomics: bitwise reproducible.
 * A row index out of range (nn, or a table that belongs to another cloud) is never followed: the rows it
 * touches come out as NaN.  Refused before any launch (PCC_ERR_ARG, the message names the argument): h or
 * radius outside 1..8, a capacity that is no power of two, null required pointers, no output at all, a short
 * scratch, n_d == 0 with n_r > 0.  n_r == 0 is valid and zeroes sums.
 * ------------------------------------------------------------------------------------- */
int pcc_surface_variation(const int32_t* coords, int64_t n, const uint64_t* keys, const int32_t* vals, int64_t cap,
                          int32_t tensor_stride, int32_t radius, double* kappa, void* stream);
int64_t pcc_pcqm_scratch_bytes(int64_t n);
int pcc_pcqm_features(const int32_t* coords_r, int64_t n_r, const uint64_t* keys_r, const int32_t* vals_r, int64_t cap_r,
                      const int32_t* coords_d, int64_t n_d, const uint64_t* keys_d, const int32_t* vals_d, int64_t cap_d,
                      int32_t tensor_stride, const int32_t* nn, const double* attrs_r, const double* attrs_d,
                      const double* w, int32_t h, const double* constants, double* stats, double* features, double* sums,
                      void* scratch, int64_t scratch_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * View rendering and view metrics of the view-dependent / region-of-interest evaluation
 * (evaluate_view_dep.py:102-305).
 *
 * pcc_render_view replaces render_pointviews (evaluate_view_dep.py:308-348, an open3d OpenGL window) by an
 * exact orthographic z-buffer splat of ONE voxelised cloud along a signed coordinate axis (every view of
 * evaluate_view_dep.py:46-57 is one).  coords [n,4] (the batch column is ignored), rgb8 uint8 [n,3];
 * right / up / front: HOST int32[3], signed unit axes, mutually orthogonal, right == up x front; front points
 * from the object to the camera (open3d's set_front).  For a row p: u = right.p, v = up.p, d = front.p; the
 * point covers columns (u - u_min) * scale + ox + i and rows (v_max - v) * scale + oy + j for i, j in
 * [0, point_size); pixels outside the image are dropped one by one (no wrap, a partly visible point is not
 * rejected whole).  A pixel shows the point with the largest d and, among equal d, the lowest row index;
 * untouched pixels show `background` (HOST, 3 bytes).  scratch: the z-buffer, uint64 [H*W] =
 * pcc_render_scratch_bytes(H, W) bytes (0 for a size the call refuses); image: uint8 [H,W,3].  All integer and
 * bitwise reproducible: the splat is a 64-bit atomic maximum of ((d + 2^18) << 32) | (0xFFFFFFFF - row), which
 * does not depend on arrival order.  A row with a coordinate beyond PCC_COORD_LIMIT draws nothing.
 * Refused before any launch (PCC_ERR_ARG): vectors that are no signed unit axes or not orthogonal, right !=
 * up x front, scale outside 1..64, point_size outside 1..16, H or W outside 1..8192, n above 2^32 - 2, a null
 * cloud with n > 0, a null or short z-buffer, a null image.  n == 0 is valid: every pixel is background.
 *
 * pcc_image_compare replaces skimage's rgb2yuv, peak_signal_noise_ratio and structural_similarity
 * (evaluate_view_dep.py:196-204, 243-249, 288-294) by their raw sums in float64 for two uint8 [H,W,3] images,
 * the reference view and the test view.  Per pixel and channel f = byte / 255.0 and YUV = (f_r m0 + f_g m1) +
 * f_b m2 with skimage's yuv_from_rgb rows, separate multiplies and adds.  out (device double[8]): [0..2] the
 * per-channel sums of squared differences over all pixels, [3..5] the per-channel sums of the SSIM map of
 * structural_similarity(win_size=7, data_range=1.0, gaussian_weights=False, use_sample_covariance=True) over
 * its crop, the interior (H-6) x (W-6) (7 x 7 window means of X, Y, XX, YY, XY; variances and covariance
 * 49/48 (mean of product - product of means); C1 = 1e-4, C2 = 9e-4; S = ((2 ux uy + C1)(2 vxy + C2)) /
 * ((ux^2 + uy^2 + C1)(vx + vy + C2))), [6] and [7] the smallest and the largest YUV value of `ref`.
 * Workgroups own pcc_image_compare_tile() x pcc_image_compare_tile() pixels and store their partial sums in
 * workgroup order in scratch (pcc_image_compare_scratch_bytes(H, W) bytes; 0 for a size the call refuses); a
 * final pass adds them in ascending order.  No float atomics: bitwise reproducible.  Refused before any
 * launch: H or W below 7 or above 8192, null pointers, a short scratch.
 *
 * pcc_view_visibility answers "which points did that image show?" for the view pcc_render_view would draw
 * (the same axes, framing, splat, clipping and winner rule; no colours, no image).  For every row i:
 *   behind[i] = the minimum, over the pixels of the row's splat that lie inside the image, of
 *               d_win(pixel) - d_i, where d_win is the largest d splatted onto the pixel.  Always >= 0; 0 exactly
 *               when the point lies on the z-buffer front in at least one of its pixels; at most 2 *
 *               PCC_COORD_LIMIT.  PCC_VIS_OFFSCREEN when no pixel of the splat lies inside the image, and for a
 *               row with a coordinate beyond PCC_COORD_LIMIT (which draws nothing, as in the renderer).
 *   won[i]    = the number of pixels whose winner is row i under the renderer's full rule (largest d, then the
 *               lowest row index).  won[i] > 0 implies behind[i] == 0; the converse fails for a point that ties
 *               the front depth in all its pixels but loses every tie.  `behind` does not depend on the tie
 *               rule (it compares depths only) and so not on the row order; `won` does.
 * accumulate != 0 folds the view into what the arrays hold: behind[i] = min(old, new), won[i] = old + new (the
 * caller has initialised them, e.g. by a first call with accumulate == 0, which overwrites).  scratch: the
 * z-buffer, pcc_visibility_scratch_bytes(H, W) = pcc_render_scratch_bytes(H, W) bytes (0 for a size the call
 * refuses).  Three launches: clear, the renderer's splat, and one thread per point that walks its splat again
 * and reads the words: that thread owns its row's outputs, so there are no atomics beyond the splat's maximum
 * and both outputs are bitwise reproducible.  Refused before any launch (PCC_ERR_ARG) on pcc_render_view's
 * conditions: bad axes, scale outside 1..64, point_size outside 1..16, H or W outside 1..8192, n above
 * 2^32 - 2, a null cloud or null outputs with n > 0, a null or short z-buffer.  n == 0 is valid, launches
 * nothing and touches no array.  Not a camera: orthographic, axis views only, square splats.
 *
 * pcc_render_camera and pcc_camera_visibility are those two operators for a PINHOLE CAMERA at a position.  The
 * camera crosses this interface as integers only (HOST arrays and scalars), and no kernel uses floating point:
 *   pos_q   int32[3]    rint(16 position): 1/16 voxel, |pos_q| <= 2^24 (2^20 voxels)
 *   axes_q  int32[3][3] rint(2^14 [right; up; front]), row-major, every entry in [-2^14, 2^14]; front points from
 *                       the scene to the camera (open3d's set_front), right = up x front
 *   focal_q int32       rint(16 focal), focal in pixels: 1 .. 2^20
 *   near_q  int32       rint(16 near), 1/16 voxel: >= 1
 *   H, W    int32       1 .. 8192
 *   ps_q    int32       rint(16 point_size), the voxel's edge in 1/16 voxel: 1 .. 256
 * For a row p (|coordinate| <= PCC_COORD_LIMIT, else it draws nothing), in int64:
 *   e = 16 p - pos_q;  U = right_q . e;  V = up_q . e;  D = -(front_q . e)         (D: depth, 2^-18 voxel)
 *   drawn <=> D >= near_q 2^14 (a point behind the camera is not drawn)
 *   X = floor(focal_q U / D);  Y = floor(focal_q V / D)                (1/16 pixel from the principal point (W/2, H/2))
 *   s = clamp(ceil(focal_q ps_q 2^10 / D), 1, 16)                                (the projected voxel edge, pixels)
 *   col0 = floor((8 W + X - 8 s) / 16);  row0 = floor((8 H - Y - 8 s) / 16)
 *   the splat covers columns col0 .. col0 + s - 1 and rows row0 .. row0 + s - 1; pixels outside the image are
 *   dropped one by one;  dk = D >> 10 (depth key, 1/256 voxel, 16 <= dk < 2^30)
 * Division rounds as written (floor towards -inf, ceil towards +inf).  |focal_q U| < 2^60 under the limits above
 * (|U| <= 3 2^14 (2^24 + 16 PCC_COORD_LIMIT) < 2^40); the entries recompute the bound from their arguments and refuse
 * a camera that would break it.  A pixel shows the drawn point with the smallest dk and, among equal dk, the lowest
 * row index: a 64-bit atomic maximum of ((0x7FFFFFFF - dk) << 32) | (0xFFFFFFFF - row) on pcc_render_view's z-buffer
 * (pcc_render_scratch_bytes(H, W) bytes), cleared and resolved by pcc_render_view's kernels.  At most s^2 <= 256
 * atomics per point.  Bitwise reproducible.
 * pcc_render_camera: coords [n,4] (batch ignored), rgb8 uint8 [n,3], background HOST 3 bytes, image uint8 [H,W,3];
 * n == 0 is valid (every pixel is background).
 * pcc_camera_visibility, for every row i (one thread walks its splat again; no atomics beyond the splat's):
 *   behind[i] = the minimum over the row's pixels inside the image of (dk_i - dk_front(pixel)) >> 8: whole voxels
 *               behind the z-buffer front; 0 = within one voxel of it.  Always >= 0.
 *   won[i]    = the number of pixels whose word is the row's own; won[i] > 0 implies behind[i] == 0.
 *   depth[i]  = dk_i.
 *   A row that is not drawn, or whose splat lies wholly outside the image: behind = depth = PCC_VIS_OFFSCREEN, won = 0.
 * accumulate != 0 folds into what the arrays hold: min / sum / min.  n == 0 launches nothing and touches no array.
 * Both refuse before any launch (PCC_ERR_ARG): a null pointer (cloud or outputs with n > 0, camera arrays,
 * background, z-buffer, image), a short z-buffer, any value outside the table above, n above 2^32 - 2.  Not a lens
 * model: no distortion, square splats, no anti-aliasing, and holes open once a voxel projects beyond 16 pixels.
 *
 * pcc_view_buffers and pcc_camera_buffers expose the z-buffer those views draw (the arguments of pcc_view_visibility /
 * pcc_camera_visibility without `accumulate`; clear, splat, then one thread per pixel):
 *   index[H,W] = the row the pixel shows under the renderer's full winner rule, -1 for background
 *   depth[H,W] = d = front . p of that row for the orthographic view, its depth key dk for the camera;
 *                PCC_VIS_OFFSCREEN for background
 * n == 0 is valid: every pixel is background.  Refused before any launch as their visibility counterparts, and on a
 * null index or depth.
 *
 * pcc_view_sample and pcc_camera_sample carry an image BACK to the points (screen-space quality maps): the clear and
 * splat of the visibility entries, then one thread per point walks its clipped splat again.  image: int32
 * [H,W,channels], channels 1 .. PCC_SAMPLE_MAX_CHANNELS.  A pixel of row i's splat COUNTS for row i when
 *   tolerance == PCC_SAMPLE_OWN: its word is row i's own (the pixels that show the point; their number is `won`);
 *   tolerance >= 0: (d_win(pixel) - d_i) <= tolerance for the view, (dk_i - dk_front(pixel)) >> 8 <= tolerance for the
 *                   camera: the quantity whose minimum over the splat is `behind`, so the pixel looks at the surface
 *                   the point belongs to, within `tolerance` whole voxels, and count[i] > 0 <=> behind[i] <= tolerance.
 * Per row, over the counted pixels:
 *   total[n,channels] int64 = the sum of the image;  count[n] int32 = their number;
 *   peak[n,channels]  int32 = the maximum, PCC_SAMPLE_NONE when nothing counted.
 * A row that is not drawn, or whose splat lies wholly outside the image: count 0, total 0, peak PCC_SAMPLE_NONE.
 * accumulate != 0 folds into what the arrays hold: sum / sum / max (a thread owns its row: a plain read-modify-write).
 * At most 256 pixels count per row and call, so |total| grows by less than 2^39 per call.  All integer, bitwise
 * reproducible, no atomics beyond the splat's.  n == 0 launches nothing and touches no array.  Refused before any
 * launch: the visibility entries' conditions, channels outside 1 .. 4, tolerance below -1, a null image, null outputs
 * with n > 0.  Not a texture unit: no sub-pixel or bilinear sampling, integer images only.
 *
 * pcc_image_compare_masked is pcc_image_compare restricted to a region: mask uint8 [H,W], nonzero = inside.  out[0..2]
 * run over the masked pixels only, out[3..5] over the windows of the crop whose centre pixel (top-left + 3, + 3) is
 * masked; out[6], out[7] stay over the whole of `ref` (the data-range rule does not change with the mask).  The same
 * tile kernel, so the additions happen in the same order: with an all-nonzero mask out[0..5] equal
 * pcc_image_compare's bit for bit.  The caller divides by the numbers of masked pixels and windows.  Refused as
 * pcc_image_compare, and on a null mask.
 * ------------------------------------------------------------------------------------- */
#define PCC_VIS_OFFSCREEN 2147483647
#define PCC_SAMPLE_MAX_CHANNELS 4
#define PCC_SAMPLE_OWN (-1)
#define PCC_SAMPLE_NONE (-2147483648)
int64_t pcc_render_scratch_bytes(int32_t H, int32_t W);
int pcc_render_view(const int32_t* coords, const uint8_t* rgb8, int64_t n, const int32_t* right, const int32_t* up,
                    const int32_t* front, int32_t u_min, int32_t v_max, int32_t ox, int32_t oy, int32_t scale,
                    int32_t point_size, int32_t H, int32_t W, const uint8_t* background, void* scratch,
                    int64_t scratch_bytes, uint8_t* image, void* stream);
int64_t pcc_visibility_scratch_bytes(int32_t H, int32_t W);
int pcc_view_visibility(const int32_t* coords, int64_t n, const int32_t* right, const int32_t* up,
                        const int32_t* front, int32_t u_min, int32_t v_max, int32_t ox, int32_t oy, int32_t scale,
                        int32_t point_size, int32_t H, int32_t W, void* scratch, int64_t scratch_bytes,
                        int32_t accumulate, int32_t* behind, int32_t* won, void* stream);
int pcc_render_camera(const int32_t* coords, const uint8_t* rgb8, int64_t n, const int32_t* pos_q,
                      const int32_t* axes_q, int32_t focal_q, int32_t near_q, int32_t H, int32_t W, int32_t ps_q,
                      const uint8_t* background, void* scratch, int64_t scratch_bytes, uint8_t* image,
                      void* stream);
int pcc_camera_visibility(const int32_t* coords, int64_t n, const int32_t* pos_q, const int32_t* axes_q,
                          int32_t focal_q, int32_t near_q, int32_t H, int32_t W, int32_t ps_q, void* scratch,
                          int64_t scratch_bytes, int32_t accumulate, int32_t* behind, int32_t* won,
                          int32_t* depth, void* stream);
int32_t pcc_image_compare_tile(void);
int64_t pcc_image_compare_scratch_bytes(int32_t H, int32_t W);
int pcc_image_compare(const uint8_t* ref, const uint8_t* img, int32_t H, int32_t W, void* scratch,
                      int64_t scratch_bytes, double* out, void* stream);
int pcc_image_compare_masked(const uint8_t* ref, const uint8_t* img, const uint8_t* mask, int32_t H, int32_t W,
                             void* scratch, int64_t scratch_bytes, double* out, void* stream);
int pcc_view_buffers(const int32_t* coords, int64_t n, const int32_t* right, const int32_t* up, const int32_t* front,
                     int32_t u_min, int32_t v_max, int32_t ox, int32_t oy, int32_t scale, int32_t point_size,
                     int32_t H, int32_t W, void* scratch, int64_t scratch_bytes, int32_t* index, int32_t* depth,
                     void* stream);
int pcc_camera_buffers(const int32_t* coords, int64_t n, const int32_t* pos_q, const int32_t* axes_q, int32_t focal_q,
                       int32_t near_q, int32_t H, int32_t W, int32_t ps_q, void* scratch, int64_t scratch_bytes,
                       int32_t* index, int32_t* depth, void* stream);
int pcc_view_sample(const int32_t* coords, int64_t n, const int32_t* right, const int32_t* up, const int32_t* front,
                    int32_t u_min, int32_t v_max, int32_t ox, int32_t oy, int32_t scale, int32_t point_size, int32_t H,
                    int32_t W, void* scratch, int64_t scratch_bytes, int32_t accumulate, const int32_t* image,
                    int32_t channels, int32_t tolerance, int64_t* total, int32_t* count, int32_t* peak, void* stream);
int pcc_camera_sample(const int32_t* coords, int64_t n, const int32_t* pos_q, const int32_t* axes_q, int32_t focal_q,
                      int32_t near_q, int32_t H, int32_t W, int32_t ps_q, void* scratch, int64_t scratch_bytes,
                      int32_t accumulate, const int32_t* image, int32_t channels, int32_t tolerance, int64_t* total,
                      int32_t* count, int32_t* peak, void* stream);

/* ---------------------------------------------------------------------------------------
 * Entropy model, device side (compressai EntropyBottleneck / GaussianConditional,
 * model/entropy_models.py:313,330,352-353,371-372,393,407-408).  Features are [N, C]
 * row-major; symbol / index / likelihood planes are channel-major [C, N] — the order in
 * which the reference flattens (1, C, N) tensors into one rANS stream.
 * ------------------------------------------------------------------------------------- */
/* symbols[c,n] = rint(z[n,c] - median[c]);  z_hat[n,c] = symbols + median  (either may be NULL). */
int pcc_eb_quantize(const float* z, int64_t n, int32_t c, const float* medians, int32_t* symbols,
                    float* z_hat, void* stream);
/* z_hat[n,c] = symbols[c,n] + median[c] */
int pcc_eb_dequantize(const int32_t* symbols, int64_t n, int32_t c, const float* medians,
                      float* z_hat, void* stream);
/* Factorized-density likelihood max(|sigmoid(s*u) - sigmoid(s*l)|, 1e-9) of v = z_hat
 * (B.2).  eb_params: per channel 58 floats = softplus(matrix_i), bias_i, tanh(factor_i)
 * flattened in the order m0[3] b0[3] f0[3] m1[9] b1[3] f1[3] m2[9] b2[3] f2[3] m3[9] b3[3]
 * f3[3] m4[3] b4[1].  lik is [C, N]. */
int pcc_eb_likelihood(const float* z_hat, int64_t n, int32_t c, const float* eb_params, float* lik,
                      void* stream);
/* params [N, 2C] = (scales | means) rows aligned with y (h_s output looked up at y's
 * coordinates).  indexes[c,n] = 63-level table index of max(scale, 0.11);
 * symbols[c,n] = rint(y - mean).  scale_table: `levels` ascending floats. */
int pcc_gc_encode_prep(const float* y, const float* params, int64_t n, int32_t c,
                       const float* scale_table, int32_t levels, int32_t* symbols,
                       int32_t* indexes, void* stream);
/* The same preparation with the planes the host coder reads directly, already in stream order: output column j
 * takes row perm[j] (perm may be NULL = identity; the reference sorts its tensors canonically before coding,
 * utils.py:155-180, model/entropy_models.py:357-372), symbols as int16 [c,n] (may be NULL: indexes only, the
 * decoder's case), indexes as uint8 [c,n] (levels <= 256).  *overflow (device int32, required with symbols) is
 * set to 1 when a symbol does not fit int16 — the caller then uses pcc_gc_encode_prep. */
int pcc_gc_encode_prep_packed(const float* y, const float* params, int64_t n, int32_t c,
                              const float* scale_table, int32_t levels, const int32_t* perm,
                              int16_t* symbols, uint8_t* indexes, int32_t* overflow, void* stream);
int pcc_gc_dequantize_i16(const int16_t* symbols, const float* params, int64_t n, int32_t c,
                          float* y_hat, void* stream);
/* y_hat[n,c] = symbols[c,n] + mean[n,c]  (GaussianConditional.decompress/dequantize). */
int pcc_gc_dequantize(const int32_t* symbols, const float* params, int64_t n, int32_t c, float* y_hat,
                      void* stream);
/* eval-mode forward: y_hat = rint(y - mean) + mean, lik[c,n] = Gaussian bin mass, floor 1e-9. */
int pcc_gc_forward(const float* y, const float* params, int64_t n, int32_t c, float* y_hat, float* lik,
                   void* stream);

/* ---------------------------------------------------------------------------------------
 * Entropy coder, host side (compressai _CXX / ans: encode_with_indexes,
 * decode_with_indexes, pmf_to_quantized_cdf — same argument order).  All pointers HOST.
 * cdfs is [n_cdfs, cdf_stride] int32.  One rANS stream per call.
 * ------------------------------------------------------------------------------------- */
/* Returns bytes written (>= 8), PCC_ERR_ARG if out_cap is too small (needs <= 4*(3n+4)). */
int64_t pcc_rans_encode_with_indexes(const int32_t* symbols, const int32_t* indexes, int64_t n,
                                     const int32_t* cdfs, int32_t cdf_stride, const int32_t* cdf_sizes,
                                     const int32_t* offsets, uint8_t* out, int64_t out_cap);
int pcc_rans_decode_with_indexes(const uint8_t* data, int64_t nbytes, const int32_t* indexes, int64_t n,
                                 const int32_t* cdfs, int32_t cdf_stride, const int32_t* cdf_sizes,
                                 const int32_t* offsets, int32_t* out_symbols);
/* The same coder on the packed planes of pcc_gc_encode_prep_packed (int16 symbols, uint8 indexes): identical
 * bytes.  The decoder sets *narrowed (host int32, required) to 1 when a decoded symbol does not fit int16 —
 * out_symbols is then unusable and the caller repeats the decode with pcc_rans_decode_with_indexes. */
int64_t pcc_rans_encode_with_indexes_i16u8(const int16_t* symbols, const uint8_t* indexes, int64_t n,
                                           const int32_t* cdfs, int32_t cdf_stride, const int32_t* cdf_sizes,
                                           const int32_t* offsets, uint8_t* out, int64_t out_cap);
int pcc_rans_decode_with_indexes_u8i16(const uint8_t* data, int64_t nbytes, const uint8_t* indexes, int64_t n,
                                       const int32_t* cdfs, int32_t cdf_stride, const int32_t* cdf_sizes,
                                       const int32_t* offsets, int16_t* out_symbols, int32_t* narrowed);
/* cdf has n+1 entries. */
int pcc_pmf_to_quantized_cdf(const float* pmf, int32_t n, int32_t precision, int32_t* cdf);

/* ---------------------------------------------------------------------------------------
 * The lane-parallel y stream "PCL1" (opt-in).  The symbol sequence is dealt to
 * `lanes` lanes (lane s owns positions s, s + lanes, ...) and lane s's substream is exactly
 * what pcc_rans_encode_with_indexes writes for that subsequence alone.  Container, little-
 * endian: "PCL1", lanes (uint16, 1 .. 4096), uint16 0, lanes x uint32 byte length (0, or a
 * multiple of 4 that is >= 8), then the substreams in lane order.
 * ------------------------------------------------------------------------------------- */
/* Checks a container's header (magic, lane count, length rules, lengths add up to nbytes):
 * the lane count, or PCC_ERR_DATA.  HOST pointer. */
int64_t pcc_rans_lanes_header(const uint8_t* data, int64_t nbytes);
/* Host twin of the GPU coder; all pointers HOST.  Encode returns the bytes written
 * (<= 8 + 4*lanes + 8*n + 16*lanes); decode checks the header, that every lane ends at state
 * 2^31 and at the end of its substream (PCC_ERR_DATA otherwise), and never reads outside data. */
int64_t pcc_rans_lanes_encode_host(const int32_t* symbols, const int32_t* indexes, int64_t n, int32_t lanes,
                                   const int32_t* cdfs, int32_t cdf_stride, const int32_t* cdf_sizes,
                                   const int32_t* offsets, uint8_t* out, int64_t out_cap);
int pcc_rans_lanes_decode_host(const uint8_t* data, int64_t nbytes, const int32_t* indexes, int64_t n,
                               const int32_t* cdfs, int32_t cdf_stride, const int32_t* cdf_sizes,
                               const int32_t* offsets, int32_t* out_symbols);
/* The coding tables of the kernels below, built on the HOST into `out` (pcc_rans_lanes_tables_bytes
 * of it; n_tables <= 256); the caller copies the blob to 16-byte aligned device memory and keeps
 * it while the tables stand. */
int64_t pcc_rans_lanes_tables_bytes(const int32_t* cdf_sizes, int32_t n_tables);
int pcc_rans_lanes_tables_build(const int32_t* cdfs, int32_t cdf_stride, const int32_t* cdf_sizes,
                                const int32_t* offsets, int32_t n_tables, void* out, int64_t out_bytes);
/* GPU encoder: symbols / indexes are DEVICE int32 sequences of n < 2^27 in stream order, `tables`
 * the device copy of the blob.  Writes the container to `out` (device, 4-byte aligned,
 * pcc_rans_lanes_encode_out_bytes of it) and result[0] = its size in bytes, result[1] = flags
 * (device int32[2]): bit 0 = a lane outgrew its share of the scratch, nothing was written past
 * it and `out` is unusable: repeat the call with worst_case = 1 (the first-guess scratch holds
 * 2 bytes per symbol); bit 1 = table index out of range, bit 2 = symbol of frequency 0, bit 3 =
 * `tables` is not a table blob.  scratch: device, pcc_rans_lanes_encode_scratch_bytes of it. */
int64_t pcc_rans_lanes_encode_scratch_bytes(int64_t n, int32_t lanes, int32_t worst_case);
int64_t pcc_rans_lanes_encode_out_bytes(int64_t n, int32_t lanes, int32_t worst_case);
int pcc_rans_lanes_encode(const int32_t* symbols, const int32_t* indexes, int64_t n, int32_t lanes,
                          const void* tables, int32_t worst_case, void* scratch, int64_t scratch_bytes,
                          uint8_t* out, int64_t out_cap, int32_t* result, void* stream);
/* GPU decoder: `data_host` and `data` are the HOST and the DEVICE (4-byte aligned) copy of one
 * container of nbytes; the header is checked on the host copy before anything is launched
 * (PCC_ERR_DATA).  indexes: device int32 [n]; out_symbols: device int32 [n] (the [C, N] plane
 * pcc_gc_dequantize reads).  *status (device int32) is 0 after a clean decode; bit 4 = a lane did
 * not end at state 2^31 and the end of its substream, bits 1 and 3 as above.  Reads of the stream
 * are clamped to each lane's substream. */
int pcc_rans_lanes_decode(const uint8_t* data_host, const uint8_t* data, int64_t nbytes, const int32_t* indexes,
                          int64_t n, const void* tables, int32_t* out_symbols, int32_t* status, void* stream);

/* ---------------------------------------------------------------------------------------
 * Code length on the device (DESIGN.md "Target-rate coding"; csrc/code_length.hip): what the
 * range coder above spends on a symbol sequence under the coding tables, in exact integers,
 * without a plane, a sort or a host step.
 *
 * cost: [n_tables, cdf_stride] int32 of Q16 bits, built on the HOST by
 * pcc_code_length_tables_build from the tables the coder takes: slot v <= cdf_sizes[t] - 2 of
 * table t holds round(65536 * (16 - log2(freq))), freq = the low 16 bits of cdf[v+1] - cdf[v]
 * as the coder reads it, float64 arithmetic; slot cdf_sizes[t] - 2 is the escape symbol; a
 * frequency of 0 (which the coder refuses) and the unused tail of a row hold -1.
 *
 * A symbol s under table t costs, with v = s - offsets[t] and maxv = cdf_sizes[t] - 2:
 * cost[t][v] when 0 <= v < maxv, else cost[t][maxv] + 4 * 65536 * (nb + nb / 15 + 1) with nb the
 * number of 4-bit nibbles of raw = -2v - 1 (v < 0) or 2 (v - maxv): every bypass put codes 4 bits.
 *
 * out: DEVICE int64 [c + 3], zeroed by the call: out[0 .. c-1] Q16 bits per channel, out[c] the
 * coder operations (symbols + bypass puts), out[c+1] the escapes, out[c+2] flags: bit 1 = table
 * index out of range (or a cdf_sizes entry outside 2 .. cdf_stride), bit 2 = a slot of frequency
 * 0 was hit, as in the lane coder.  With a flag set the sums are unspecified; nothing is read
 * out of bounds.  Sums are integer atomics: two runs agree bit for bit.  1 <= c <= 4096.
 * ------------------------------------------------------------------------------------- */
int pcc_code_length_tables_build(const int32_t* cdfs, int32_t cdf_stride, const int32_t* cdf_sizes,
                                 int32_t n_tables, int32_t* out);
/* y [N, C] under params [N, 2C]: the symbols and indexes of pcc_gc_encode_prep, never written.
 * cost / cdf_sizes / offsets (DEVICE) hold one table per scale level (`levels` of them). */
int pcc_gc_code_length(const float* y, const float* params, int64_t n, int32_t c,
                       const float* scale_table, int32_t levels, const int32_t* cost,
                       int32_t cdf_stride, const int32_t* cdf_sizes, const int32_t* offsets,
                       int64_t* out, void* stream);
/* z [N, C]: the symbols of pcc_eb_quantize, table index = channel (c tables). */
int pcc_eb_code_length(const float* z, int64_t n, int32_t c, const float* medians, const int32_t* cost,
                       int32_t cdf_stride, const int32_t* cdf_sizes, const int32_t* offsets,
                       int64_t* out, void* stream);
/* int32 planes [c, n] (channel-major, any column order: the sums do not depend on it). */
int pcc_code_length_planes(const int32_t* symbols, const int32_t* indexes, int64_t n, int32_t c,
                           const int32_t* cost, int32_t cdf_stride, const int32_t* cdf_sizes,
                           const int32_t* offsets, int32_t n_tables, int64_t* out, void* stream);

/* ---------------------------------------------------------------------------------------
 * RAHT, the region-adaptive hierarchical transform (de Queiroz & Chou 2016): the attribute
 * transform of the octree + RAHT anchor codec (DESIGN.md "Anchor codec").  csrc/raht.hip.
 *
 * Rows are the n distinct voxels of one cloud in ascending Morton order of (c - origin) over
 * `depth` bits per axis: key bit 3b+2 is x's bit b, 3b+1 y's, 3b z's (the child index
 * (x<<2)|(y<<1)|z of pcc_octree_occupancy; pcc_octree_expand's output is in row order).
 * There are 3*depth steps, s = 0 (the finest key bit) upward.  At step s two nodes whose keys
 * agree in key >> (s+1) merge: the left one (bit s = 0) has w0 points and value a0, the right
 * one w1 and a1; per channel, in float64, each operation rounded separately:
 *     low  = (sqrt(w0)*a0 + sqrt(w1)*a1) / sqrt(w0+w1)
 *     high = (sqrt(w0)*a1 - sqrt(w1)*a0) / sqrt(w0+w1)
 * `low` stays in the first row of the left node, `high` goes to the first row of the right
 * node and is final; a node without a sibling passes up unchanged.  Afterwards row 0 holds
 * the DC and every other row one high-pass coefficient.  The inverse runs the steps top first:
 *     a0 = (sqrt(w0)*low - sqrt(w1)*high) / sqrt(w0+w1)
 *     a1 = (sqrt(w1)*low + sqrt(w0)*high) / sqrt(w0+w1)
 * No atomics touch the values: the result is bitwise reproducible.
 * ------------------------------------------------------------------------------------- */
int64_t pcc_raht_scratch_bytes(int64_t n);
/* The plan of coords [n,4] int32 (batch column ignored), n >= 1, 0 <= depth <= 17; origin is
 * a HOST int32[3], everything else DEVICE.  Outputs, int32: perm[n] = input row of every
 * Morton row; per row i > 0 step[i] = index of the highest set bit of key[i] ^ key[i-1] (the
 * one step at which row i receives its coefficient), left[i] = the first row whose
 * key >> (step+1) equals row i's (its partner), w0[i] = i - left[i], w1[i] = the number of rows
 * from i on that share row i's key >> step; row 0 has step -1, left 0, w0 = w1 = 0.
 * step_rows[n] = the rows in order of (step, row), the rows without a step last;
 * step_offsets[3*depth+1]: step s owns step_rows[step_offsets[s] .. step_offsets[s+1]).
 * status[0] = rows outside the grid [origin, origin + 2^depth)^3 (their key is 0), status[1] =
 * rows whose voxel an earlier row holds (they get step -1 and left = their own row); when
 * either is non-zero the plan describes no transform.  scratch: pcc_raht_scratch_bytes(n). */
int pcc_raht_plan(const int32_t* coords, int64_t n, const int32_t* origin, int32_t depth, int32_t* perm,
                  int32_t* step, int32_t* left, int32_t* w0, int32_t* w1, int32_t* step_rows,
                  int32_t* step_offsets, int32_t* status, void* scratch, int64_t scratch_bytes, void* stream);
/* values [n,c] float64 (DEVICE, rows in Morton order, 1 <= c <= 16) transformed in place: one
 * launch per non-empty step, and one for the run of steps at the top that have at most 256
 * rows each (the same operations in the same order); inverse = 0 forward, 1 inverse.  step_offsets_host: a HOST copy of
 * the plan's step_offsets (checked: ascending from 0, at most n). */
int pcc_raht_transform(double* values, int64_t n, int32_t c, const int32_t* left, const int32_t* w0,
                       const int32_t* w1, const int32_t* step_rows, const int32_t* step_offsets_host,
                       int32_t depth, int32_t inverse, void* stream);

/* ---------------------------------------------------------------------------------------
 * Region-wise quantisation of the RAHT coefficients (the "PCR2" stream of raht.py; DESIGN.md
 * "Anchor codec: region-wise quantisation").  csrc/raht.hip.
 *
 * A quantisation LEVEL is an integer 0 .. 63; level l quantises with the step steps[l] of a
 * 64-entry table the caller supplies (raht.py: level_steps, one Gaussian-table spacing per level).
 * Blocks: the rows inside one cube of edge 2^block_log2 of the plan's grid.  In Morton row order
 * they are runs of rows, and row i opens a block iff i = 0 or step[i] >= 3*block_log2: the
 * plan alone gives the boundaries, no keys are needed.  A block's level is the MINIMUM (the
 * finest) of its points' levels.  The coefficient of row i > 0 summarises the rows
 * [left[i], i + w1[i]) and takes the minimum level among them; that range minimum equals a walk
 * over the transform's steps, finest first, on lev[] = the block level of every row:
 *     m = min(lev[left[i]], lev[i]);  coeff_level[i] = m;  lev[left[i]] = m
 * Row 0 (the DC) takes lev[0] after the last step, the minimum over the cloud.  Every
 * coefficient above a block of the finest level therefore carries that level, and the rows of
 * such a block decode exactly as under uniform coding at it.  All of it is integer min: the
 * results do not depend on any order of execution.
 * ------------------------------------------------------------------------------------- */
/* step: the plan's (DEVICE, n rows); 0 <= block_log2 <= 17 (block_log2 >= depth: one block).
 * Outputs (DEVICE): block_of_row[n] int32, ascending from 0, and n_blocks[1] int32.
 * scratch: pcc_raht_scratch_bytes(n).  Five launches (flags, three scan kernels, count). */
int pcc_raht_blocks(const int32_t* step, int64_t n, int32_t block_log2, int32_t* block_of_row,
                    int32_t* n_blocks, void* scratch, int64_t scratch_bytes, void* stream);
/* levels: uint8 [n] per point in the INPUT row order (row i of the plan reads levels[perm[i]]),
 * each 0 .. 63 -> block_level[n_blocks] int32 = the minimum over the block's rows (initialised
 * here).  A segmented min over each wave, then one integer atomicMin per (wave, block).
 * status[0] (int32, cleared here) counts the levels above 63; they are read as 63. */
int pcc_raht_block_levels(const uint8_t* levels, const int32_t* perm, const int32_t* block_of_row,
                          int64_t n, int64_t n_blocks, int32_t* block_level, int32_t* status,
                          void* stream);
/* block_level [n_blocks] int32 (values outside 0 .. 63 are clamped) -> coeff_level[n] uint8 by
 * the walk above, on the launch plan of pcc_raht_transform: one launch per non-empty step, the
 * top steps of at most 256 rows each in one workgroup, which also writes the DC's level.  No
 * atomics.  lev: int32 [n] of scratch (the walk's working array).  step_offsets_host as for
 * pcc_raht_transform, checked the same way. */
int pcc_raht_coeff_levels(const int32_t* block_level, const int32_t* block_of_row, int64_t n,
                          int64_t n_blocks, const int32_t* left, const int32_t* step_rows,
                          const int32_t* step_offsets_host, int32_t depth, uint8_t* coeff_level,
                          int32_t* lev, void* stream);
/* coeffs [n,c] float64 -> symbols [n,c] int32 = rint(coeff / steps[coeff_level[row]]), ties to
 * even, the division correctly rounded.  steps_host: a HOST float64[64], every entry positive
 * and finite.  status[0] (cleared here) counts the symbols of magnitude >= 2^28 (or NaN); they
 * are written as 0. */
int pcc_raht_quantize(const double* coeffs, int64_t n, int32_t c, const uint8_t* coeff_level,
                      const double* steps_host, int32_t* symbols, int32_t* status, void* stream);
/* coeffs [n,c] float64 = symbol * steps[coeff_level[row]] (one rounding). */
int pcc_raht_dequantize(const int32_t* symbols, int64_t n, int32_t c, const uint8_t* coeff_level,
                        const double* steps_host, double* coeffs, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PCC_HIP_H */
