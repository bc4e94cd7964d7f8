/* d4w.h -- C ABI of the MI355X-native DAS4Whales hot path (libd4w.so, built for gfx950).
 *
 * This is the drop-in boundary: plain C, device pointers and sizes only, no torch / numpy types.
 * The reference (leabouffaut/DAS4Whales @ 2024_08_07) has no FFI of its own -- its hot path is a
 * set of Python module functions over NumPy arrays -- so each entry point below cites the
 * reference function (file:line under src/das4whales/) whose array arithmetic it replaces.  The
 * Python mirror of the reference namespace (das4whales_amd/dsp.py, detect.py) and any other host
 * language bind these symbols (see INTEGRATION.md for the ctypes stub a reference maintainer
 * would add).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer on the current HIP device unless its name ends in _host;
 *   - matrices are row-major [nx channels][ns time samples], float32, time fastest;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls are asynchronous
 *     with respect to the host and ordered on that stream;
 *   - return value: 0 = D4W_OK, negative = error; d4w_last_error() gives the message of the
 *     last failure on the calling thread.
 */
#ifndef D4W_H
#define D4W_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define D4W_OK 0
#define D4W_EINVAL (-1)  /* bad argument / unsupported shape */
#define D4W_ENOMEM (-2)  /* device or host allocation failed */
#define D4W_EHIP (-3)    /* HIP runtime error (message has the call) */

const char* d4w_last_error(void);
/* "d4w <version> gfx950" -- lets the host side assert that the native library is the one loaded */
const char* d4w_version(void);

/* ------------------------------------------------------------------------------------------
 * f-k filter application:  y = real(ifft2(ifftshift(fftshift(fft2(x)) * M)))
 * replaces dsp.fk_filter_filt (dsp.py:725-756) and dsp.fk_filter_sparsefilt (dsp.py:759-786);
 * also the apply half of dsp.fk_filt (dsp.py:919,948-953).
 *
 * A plan owns the factorisation of the packed 2-D transform (nx x ns/2 complex), its twiddle /
 * index tables and the folded, permuted mask.  Requirements: ns even.  nx, ns / 2: any (prime factors
 * > 31 run Bluestein convolutions: inside the LDS tiles of passes C / B while that part of nx is
 * <= 4096 and that part of ns / 2 <= 2048, in global memory -- scratch <= 1 GiB per axis owned by the
 * plan, several times slower -- beyond).  Plans are immutable after set_mask and may be shared by streams that serialise
 * their own calls.
 * ------------------------------------------------------------------------------------------ */
typedef struct d4w_fk_plan d4w_fk_plan;

int d4w_fk_plan_create(int nx, int ns, d4w_fk_plan** plan);
/* opts: NULL or 6 ints {C1, C2, N1, N2, TA, TC}; any entry <= 0 keeps the planner's choice */
int d4w_fk_plan_create_ex(int nx, int ns, const int* opts_host, d4w_fk_plan** plan);
int d4w_fk_plan_destroy(d4w_fk_plan* plan);
/* 1 when [nx][ns] runs shape-specialised kernels (every sub-transform a compile-time register butterfly), 0 when it
 * runs the generic runtime-radix passes.  Specialised configurations for further shapes are compiled on demand by the
 * host side (das4whales_amd/fkjit.py: same templates, one translation unit per shape) and handed over with
 * d4w_fk_register_shape (entry = the d4w::FkFastEntry of csrc/fk_entry.h, entry_size = its sizeof as a build guard). */
int d4w_fk_shape_is_specialised(int nx, int ns);
int d4w_fk_register_shape(const void* entry, size_t entry_size);
/* fills {nx, ns, C1, C2, N1, N2, TA, TC} */
int d4w_fk_plan_info(const d4w_fk_plan* plan, int* info8_host);

/* Mask as the reference hands it over: dense [nx][ns] float32 on the fftshift-ed (k, f) grid
 * (dsp.py:129-130,137).  Folds it to its Hermitian part M_h = (M(k,f)+M(-k,-f))/2 -- which is
 * what `.real` at dsp.py:756,786 keeps -- and stores it in the plan's internal order.
 * Synchronises `stream` (the row-liveness scan of the folded mask is read back by the host). */
int d4w_fk_set_mask_dense_f32(d4w_fk_plan* plan, const float* mask_shifted, void* stream);
/* Same, with the OPT-IN tail pruning: wavenumber rows whose folded gains all stay at or below
 * prune_eps * max|M_h| (together with their Hermitian partner row's) are treated as zero, i.e. dead
 * (see d4w_fk_plan_live_rows).  hybrid_ninf_filter_design (dsp.py:348-406) multiplies every
 * wavenumber row by Butterworth tails that never reach zero (7.7e-7 at fmax + 14 Hz), so its rows are
 * all formally alive; prune_eps = 4e-6 keeps only the rows the speed band touches.  Not exact: the
 * output changes by at most the pruned gain times the input's energy in those bins.  0 = exact. */
int d4w_fk_set_mask_dense_pruned_f32(d4w_fk_plan* plan, const float* mask_shifted, double prune_eps, void* stream);
/* A reference design written straight into the plan, with no dense mask in between: what
 * d4w_design_mask_f32(mode, ...) followed by d4w_fk_set_mask_dense_pruned_f32 leaves in the plan, bit for bit
 * (same closed forms, same float32 rounding before the fold), for the three designs that have a closed
 * form -- mode 0 dsp.fk_filter_design (dsp.py:85-171), 1 dsp.hybrid_filter_design (dsp.py:174-305),
 * 2 dsp.hybrid_ninf_filter_design (dsp.py:308-454); arguments as d4w_design_mask_f32 below.  The Gaussian-blurred
 * designs (modes 3-5) need the dense grid and are refused.  Saves the nx*ns*4-byte mask (9.6 GB at
 * 20 000 x 120 000) and its write + read.  Synchronises `stream`. */
/* dsp.fk_filt's min-max normalisation (dsp.py:945) folded into the mask upload: every value enters as
 * mask * scale + offset (scale = 1 / (max - min), offset = -min * scale, min and max from d4w_minmax_f32), exactly what
 * d4w_minmax_normalise_f32 followed by d4w_fk_set_mask_dense_f32 leaves, without the extra read and write of the mask. */
int d4w_fk_set_mask_dense_affine_f32(d4w_fk_plan* plan, const float* mask_shifted, float scale, float offset,
                                     void* stream);
int d4w_fk_set_mask_design_f32(d4w_fk_plan* plan, int mode, double k_spacing, double t_spacing,
                               const double* params8_host, int i0, int i1, const double* hrow_dev,
                               double prune_eps, void* stream);

/* Number of wavenumber rows (0..nx) the current mask keeps alive.  A row whose folded mask -- and
 * whose Hermitian partner's -- is identically zero is multiplied by zero whatever it holds; the
 * shape-specialised kernels skip such rows in the three middle passes (exact, the analogue of the
 * reference's sparse.COO product at dsp.py:782).  nx = nothing is skipped (dense mask, or a shape
 * that runs the generic kernels).  D4W_FK_NOPRUNE=1 in the environment disables the skipping. */
int d4w_fk_plan_live_rows(const d4w_fk_plan* plan);

/* Order of the five passes for the current mask (shape-specialised kernels).  The c2 and n2 sub-transforms commute, so
 * besides the channel-first order A, C, B, C', A' (which skips dead WAVENUMBER rows) the filter can run time-first:
 * A, Bf, Cm, Bi, A' with the half spectrum compacted between Bf and Bi -- frequency columns whose folded gain is zero are
 * never written, columns whose gain is the same for every wavenumber (the Butterworth skirts hybrid_ninf_filter_design
 * keeps outside its looped columns, dsp.py:348-360) are scaled in Bf and skip the channel transform, the others go
 * through Cm (c2 forward x mask x c2 inverse in one visit).  Exact like the channel-first order: both treat as zero only
 * gains below max(prune_eps, 2^-24 / sqrt(nx ns)) * max|M_h| -- at prune_eps = 0 at most half a float32 ulp of the
 * input's RMS in any output sample (D4W_FK_ROUND_EPS=0: exact zeros only).  The plan picks the order that moves fewer
 * bytes (D4W_FK_ORDER=cf|tf forces one).  info6 = {1 time-first / 0 channel-first, band columns kept per row, tail
 * columns kept per row, ns / 2, live wavenumber rows, nx}; bytes2 = modelled bytes per channel-sample {channel-first,
 * time-first}. */
int d4w_fk_plan_order(const d4w_fk_plan* plan, int* info6_host, double* bytes2_host);

/* x -> y (may alias).  taper != 0 multiplies x by tukey(ns, 0.03) first (dsp.taper_data,
 * dsp.py:705-722, fused into the first pass; x itself is not modified). */
int d4w_fk_apply_f32(d4w_fk_plan* plan, const float* x, float* y, int taper, void* stream);

/* d4w_fk_apply_f32 that also returns what the matched filter normalises the filtered rows by
 * (detect.py:157): row_mean[c] = mean(y[c,:]) DEVICE float64 [nx] (the reference de-means in float64; the correlators
 * take it as a two-float value), row_maxabs[c] = max|y[c,:]| DEVICE float32 [nx].
 * The shape-specialised kernels form them in the epilogue of the last pass (no extra read of y);
 * other shapes run d4w_row_stats_f32 afterwards.  Feed them to d4w_xcorr_fft_f32 / d4w_xcorr_lens_f32. */
int d4w_fk_apply_stats_f32(d4w_fk_plan* plan, const float* x, float* y, int taper, double* row_mean,
                           float* row_maxabs, void* stream);
/* 1 when d4w_fk_apply_stats_f32 on this plan forms the statistics in the last pass's epilogue, 0 when it sweeps y afterwards
 * (small pass tiles on large blocks, the 60-s file shapes; unspecialised shapes): a caller that also wants the rows' prefix
 * maxima then runs d4w_fk_apply_f32 + d4w_row_stats_prefix_f32 for the same traffic. */
int d4w_fk_stats_in_epilogue(const d4w_fk_plan* plan);

/* Same as d4w_fk_apply_f32 but brackets each of the five passes (A, C, B, C', A') with HIP events
 * on `stream`, synchronises, and returns their durations in milliseconds in ms5_host[0..4].
 * Measurement aid for bench.py's roofline report; not for production loops. */
int d4w_fk_apply_timed_f32(d4w_fk_plan* plan, const float* x, float* y, int taper, void* stream,
                           float* ms5_host);
/* timed variant of d4w_fk_apply_stats_f32 (row_mean / row_maxabs may both be NULL) */
int d4w_fk_apply_timed_stats_f32(d4w_fk_plan* plan, const float* x, float* y, int taper, double* row_mean,
                                 float* row_maxabs, void* stream, float* ms5_host);

/* ------------------------------------------------------------------------------------------
 * Distributed f-k filter: ONE [nx][ns] block sharded by contiguous channel block over `world`
 * GPUs (rank r owns rows [row_begin, row_end), balanced like np.array_split).  Exactly the same
 * filter as d4w_fk_apply_f32 -- the 2-D transform couples all channels, so the packed spectrum is
 * re-sharded once each way (pencil decomposition):
 *
 *   d4w_fkd_time_fwd_f32   local rows: x_loc [nxl][ns] real -> z_loc [nxl][N1][N2] complex
 *                          (time-axis transform of the packed rows; q1-major sub-rows of N2 bins)
 *   -- all-to-all: sub-row q1 of every channel goes to rank owner[q1] (d4w_fkd_plan_q1_owner);
 *      the receiver concatenates the senders' pieces in rank order = channel order, which gives
 *      slab [nx][nq][N2] (nq = sub-rows owned, in ascending q1)
 *   d4w_fkd_chan_apply_f32 channel-axis transform, real-spectrum pair op x folded mask, inverse
 *                          channel-axis transform (x 1/(nx ns/2)), in place on the slab
 *   -- all-to-all back (the exact reverse)
 *   d4w_fkd_time_inv_f32   z_loc -> filtered rows, in place (read the buffer as float [nxl][ns])
 *
 * The exchange itself (RCCL all_to_all_single over xGMI, gloo in the CPU tests) is host plumbing:
 * das4whales_amd/shard.py fk_filter_sharded.  All buffers are DEVICE float32 (complex = 2 floats).
 * info12 = {nx, ns, world, rank, row_begin, row_end, N1, N2, nq, C1, C2, packed}.
 *
 * PACKED plans (d4w_fkd_plan_is_packed; every shape with shape-specialised kernels, e.g. 20000 x 120000 and the
 * 60-s file shapes) need no repacking around the exchanges: the time phase writes straight into the send buffer,
 * destination rank major --
 *   packed = [dest rank s][local row l][jq < nq(s)][N2] complex, block s holding nxl * nq(s) * N2 elements,
 * so that all_to_all_single delivers the slab [nx][nq][N2] as it stands (senders in rank order = channel order), and
 * the second exchange delivers the same layout back:
 *   d4w_fkd_time_fwd_packed_f32   x_loc [nxl][ns] -> packed            (n1 sub-transform + four-step twiddle)
 *   d4w_fkd_chan_apply_f32        slab, in place: c1 transform, c2 transform, n2 transform + pair op x mask +
 *                                 inverse n2, inverse c2, inverse c1    (five launches of the fk_fast.h kernels)
 *   d4w_fkd_time_inv_packed_f32   packed -> y_loc [nxl][ns]
 * Seven block passes per rank over its share instead of the single-device five; the generic plan (any other
 * shape) keeps the z_loc / index-packing protocol above.  Generic plan: nx, ns / 2 any (a prime factor > 31 turns
 * the slab's channel transform / the rows' time transform into a Bluestein convolution in global memory: scratch
 * <= 1 GiB each owned by the plan, D4W_FKD_BZ_CHUNK = columns / D4W_FKD_BT_CHUNK = rows per chunk; with such an
 * ns / 2 the half spectrum is one natural-order class, N1 = 1, owned by rank 0).
 * ------------------------------------------------------------------------------------------ */
typedef struct d4w_fkd_plan d4w_fkd_plan;
int d4w_fkd_plan_create(int nx, int ns, int world, int rank, d4w_fkd_plan** plan);
int d4w_fkd_plan_destroy(d4w_fkd_plan* plan);
int d4w_fkd_plan_info(const d4w_fkd_plan* plan, int* info12_host);
int d4w_fkd_plan_q1_owner(const d4w_fkd_plan* plan, int* owner_host /* [N1] */);
/* The Bluestein channel phase transforms only the slab columns whose folded gains -- or whose Hermitian partner column's --
 * are not all zero with the mask set last (the others leave the pair op as zeros): info2 = {those, all slab columns},
 * {0, 0} when the channel phase is not the global-memory Bluestein form.  D4W_FKD_BZ_BAND=0 transforms every column. */
int d4w_fkd_plan_live_columns(const d4w_fkd_plan* plan, int* info2_host);
/* mask: the full dense [nx][ns] float32 mask on the fftshift-ed grid (as d4w_fk_set_mask_dense_f32);
 * only the owned sub-rows are folded and kept */
int d4w_fkd_set_mask_dense_f32(d4w_fkd_plan* plan, const float* mask_shifted, void* stream);
/* the closed-form designs straight into the plan (see d4w_fk_set_mask_design_f32): a rank evaluates only the
 * gains of the sub-rows it owns, so no rank ever holds the dense mask.  Bit-identical to the dense route. */
int d4w_fkd_set_mask_design_f32(d4w_fkd_plan* plan, int mode, double k_spacing, double t_spacing,
                                const double* params8_host, int i0, int i1, const double* hrow_dev, void* stream);
int d4w_fkd_time_fwd_f32(d4w_fkd_plan* plan, const float* x_loc, float* z_loc, int taper, void* stream);
int d4w_fkd_chan_apply_f32(d4w_fkd_plan* plan, float* slab, void* stream);
int d4w_fkd_time_inv_f32(d4w_fkd_plan* plan, float* z_loc, void* stream);
int d4w_fkd_plan_is_packed(const d4w_fkd_plan* plan);
int d4w_fkd_time_fwd_packed_f32(d4w_fkd_plan* plan, const float* x_loc, float* packed, int taper, void* stream);
int d4w_fkd_time_inv_packed_f32(d4w_fkd_plan* plan, const float* packed, float* y_loc, void* stream);
/* the same on local rows [l0, l1) only (l0 a multiple of C1): row chunks whose transfer overlaps the next chunk's
 * transform (das4whales_amd/shard.py) */
int d4w_fkd_time_fwd_packed_rows_f32(d4w_fkd_plan* plan, const float* x_loc, float* packed, int taper, int l0, int l1,
                                     void* stream);
int d4w_fkd_time_inv_packed_rows_f32(d4w_fkd_plan* plan, const float* packed, float* y_loc, int l0, int l1, void* stream);
/* ... also leaving mean and max|.| of the filtered local rows (what detect.compute_cross_correlogram normalises by,
 * detect.py:157) in row_mean / row_maxabs [nxl], which the caller zeroes before the first chunk */
int d4w_fkd_time_inv_packed_rows_stats_f32(d4w_fkd_plan* plan, const float* packed, float* y_loc, int l0, int l1,
                                           double* row_mean, float* row_maxabs, void* stream);

/* dsp.taper_data (dsp.py:705-722): x *= tukey(ns, 0.03) in place, every row */
int d4w_taper_f32(float* x, int nx, int ns, void* stream);

/* ------------------------------------------------------------------------------------------
 * Zero-phase IIR filtering along time (rows independent):
 * replaces dsp.bp_filt (dsp.py:859-880: butter(8,'bp') + scipy.signal.filtfilt) and the user-side
 * scipy.signal.sosfiltfilt(sos, x, axis=1) applied to dsp.butterworth_filter designs
 * (dsp.py:789-827; Example.py:55, DAS4Whales_ExampleNotebook.md:292).
 *
 * SciPy semantics kept: odd extension by `padlen` samples on both sides, every section started
 * in its steady state for the first (extended) sample (sosfilt_zi * ext[0]), forward pass,
 * backward pass started at sosfilt_zi * y_fwd[last], crop.  The cascade runs as float32
 * second-order sections (the reference's 16-pole `ba` recursion is float64-only).
 *
 * Rows are cut into time segments of `seg_len` samples that run concurrently; a segment that
 * does not start at the row edge is warmed up over `warm` samples (host-chosen from the decay
 * of the cascade's impulse response, so the truncation error is below float32 resolution).
 * seg_len <= 0 or warm <= 0: one segment per row (exact recursion over the whole row).
 *
 *   sos_host [nsec][6]  = b0 b1 b2 a0(=1) a1 a2 (scipy layout), float64, HOST memory
 *   zi_host  [nsec][2]  = scipy.signal.sosfilt_zi(sos), float64, HOST memory
 *   ws: device workspace of d4w_sosfiltfilt_ws_bytes() bytes;  y may alias x.
 * Errors: D4W_EINVAL if ns <= padlen (SciPy raises ValueError there), nsec < 1 or nsec > 10.
 * ------------------------------------------------------------------------------------------ */
size_t d4w_sosfiltfilt_ws_bytes(int nx, int ns, int padlen);
int d4w_sosfiltfilt_f32(const float* x, float* y, int nx, int ns, const double* sos_host,
                        const double* zi_host, int nsec, int padlen, int seg_len, int warm,
                        void* ws, void* stream);
/* What the calling thread's last successful d4w_sosfiltfilt_f32 / d4w_sosfiltfilt_ends*_f32 call dispatched (0 before the
 * first): lanes per row + 100 x bytes per state -- 1 = one row per lane (sos_pass), 8 or 16 = the sections of a row
 * on that many adjacent lanes (sos_pass_lanes); 400 = float states, 800 = double states (chosen from the design's conditioning
 * or by D4W_SOS_F64).  E.g. 408, 816, 401, 801.  Host bookkeeping only: for tests and diagnostics. */
int d4w_sosfiltfilt_last_form(void);
/* The two row-end pieces of every row filtered exactly and written into y -- what the overlap-save form of the band-pass
 * (d4w_fir_fft_f32: the interior) leaves to the recursion: the left piece x[r][0 .. piece) and the right piece
 * x[r][ns - piece .. ns) of every row run d4w_sosfiltfilt_f32's arithmetic as rows of `piece` samples (filtfilt's edge rule at
 * the true row end; the artificial cut at the inner end has decayed after piece - keep samples), read in place from x, and
 * their `keep` outer outputs go straight to y[r][0 .. keep) and y[r][ns - keep .. ns): no gathered copy of the pieces, no
 * scattered copy of the results.  The sections of a piece run on adjacent lanes (csrc/rowops.hip: sos_pass_lanes).
 * phase 0: both passes; 1: the forward pass only (reads x, fills ws); 2: the backward pass only (reads ws, writes y) -- a
 * caller that runs the interior kernel meanwhile orders phase 2 behind it (the interior writes columns [K, ns - K), the
 * pieces own [0, keep) and [ns - keep, ns), keep > K).  x and y must not alias; ws: d4w_sosfiltfilt_ends_ws_bytes. */
size_t d4w_sosfiltfilt_ends_ws_bytes(int nx, int piece, int padlen);
int d4w_sosfiltfilt_ends_f32(const float* x, float* y, int nx, int ns, const double* sos, const double* zi, int nsec,
                             int padlen, int piece, int keep, int phase, void* ws, void* stream);
/* The same for ONE row end: sides = 1 the left pieces only, 2 the right pieces only (3 = both = the call above) -- a file
 * whose other end continues into a neighbouring file (das4whales_amd/stream.py: the first / last file of a record takes
 * d4w_fir_fft_halo_f32 with a stand-in halo on its free side and this call for that side's `keep` columns, after it). */
int d4w_sosfiltfilt_ends_sides_f32(const float* x, float* y, int nx, int ns, const double* sos, const double* zi, int nsec,
                                   int padlen, int piece, int keep, int phase, int sides, void* ws, void* stream);

/* ------------------------------------------------------------------------------------------
 * Fused ingest (the step in front of the path): data_handle.load_das_data's channel selection and
 * float conversion + data_handle.raw2strain (data_handle.py:157-176,213-214):
 *   y[r][:] = (float64(raw[c0 + r*cstep][:]) - mean_r) * scale_factor,   r < nx_out
 * raw: DEVICE [nch][ns] row-major of raw_dtype 0 = int32 (OptaSense RawData), 1 = int16,
 * 2 = float32, 3 = float64; y: float32 [nx_out][ns].  One read of the selected raw rows, one write.
 * ------------------------------------------------------------------------------------------ */
int d4w_raw2strain_f32(const void* raw, int raw_dtype, int ns, int c0, int cstep, int nx_out,
                       double scale_factor, float* y, void* stream);

/* ------------------------------------------------------------------------------------------
 * Matched filter (time-domain cross-correlation, positive lags), rows independent:
 * replaces detect.compute_cross_correlogram (detect.py:140-166), detect.shift_xcorr
 * (detect.py:96-112) and the numerator of detect.shift_nxcorr (detect.py:115-137).
 *
 *   d4w_row_stats_f32:  mean[c] = mean(x[c,:]) as FLOAT64,  maxabs[c] = max|x[c,:]|   (detect.py:157).  The mean is
 *       accumulated about a pivot sample and kept in float64; every correlator splits it into hi + lo float32 parts and
 *       de-means as (x - hi) - lo, so a row whose offset is 10^3..10^5 x its signal is still de-meaned to float32 rounding
 *       of the signal (a float32 mean leaves |mean| 2^-24 in every sample).
 *   d4w_xcorr_f32:      for each template t < ntpl (1 or 2 per call, fused: x is read once)
 *       y_t[c][k] = g[c] * sum_{n < L_t, n+k < ns} (x[c][n+k] - m[c]) * taps[t][n]
 *       with m = mean (or 0 if mean == NULL) and g = 1/maxabs (or 1 if maxabs == NULL; 0 for an
 *       all-zero row, where the reference divides by zero).
 *   taps: DEVICE float32 [ntpl][ltaps] (ltaps multiple of 4, zero padded), the template's
 *   support already normalised by the host exactly as detect.py:158 does.
 * The de-meaned zero-padded template's DC tail (-mean/max on the padded part, detect.py:158) is a
 * separate entry point, d4w_xcorr_dc_tail_f32.
 * ------------------------------------------------------------------------------------------ */
int d4w_row_stats_f32(const float* x, int nx, int ns, double* mean, float* maxabs, void* stream);

/* dst[r][0 .. ncols) = src[r][0 .. ncols), r < nrows, rows ld_src / ld_dst floats apart (DEVICE pointers): the strided piece
 * copies around the band-pass (row ends to the recursion and back, dsp.py:859-880) in one launch each. */
int d4w_copy_cols_f32(const float* src, size_t ld_src, float* dst, size_t ld_dst, int nrows, int ncols, void* stream);
int d4w_xcorr_f32(const float* x, int nx, int ns, const double* mean, const float* maxabs,
                  const float* taps, int ntpl, int ltaps, float* y0, float* y1, void* stream);
/* Same, with the true support of each template (len_t <= ltaps, taps[t][len_t..ltaps) == 0): taps
 * beyond the shorter support are only applied to the longer template (HF 136 / LF 156 samples). */
int d4w_xcorr_lens_f32(const float* x, int nx, int ns, const double* mean, const float* maxabs,
                       const float* taps, int ntpl, int ltaps, int len0, int len1, float* y0,
                       float* y1, void* stream);

/* The constant the reference leaves on the zero-padded part of the de-meaned template (detect.py:158):
 *   y[c][k] += coef * g[c] * sum_{i < k + support} (x[c][i] - m[c]),  k + support < ns,
 * coef = mean(template) / max|template| over the zero-padded length, support = length of the non-zero
 * part.  Added in place to a correlogram produced by d4w_xcorr_*_f32 with the same mean / maxabs.
 * |coef| ~ 5e-7 for the fin-whale templates: a 3-5e-6 effect on a 60-s file of WHITE rows, 3e-8 on band-passed rows, 1e-3 on
 * rows that drift (the term is |coef| g times a PREFIX SUM of the de-meaned row: its weight is a property of the data).
 *
 * d4w_row_prefix_max_f32:  pmax[c] = max_j |sum_{i < j} (x[c][i] - m[c])|  -- the most the term of row c can reach is
 *     |coef| g[c] pmax[c]; one read of x.
 * d4w_xcorr_dc_tail_rows_f32: the same update with a per-row decision: with pmax / rowmax given (rowmax[c] = max over the
 *     lags of y[c][:], d4w_xcorr_mm_rowmax_f32's epilogue) a row with |coef| g pmax <= eps max(rowmax, 0) is left alone --
 *     the omitted term is below eps of that row's largest correlation, whatever the data --, every other row receives the
 *     term and its rowmax entry is formed again.  pmax = rowmax = NULL: every row (d4w_xcorr_dc_tail_f32).  The Python
 *     mirror runs this with eps = 1e-6 (a tenth of the parity bar) whenever a zero-padded template has a non-zero mean. */
int d4w_xcorr_dc_tail_f32(const float* x, int nx, int ns, const double* mean, const float* maxabs,
                          double coef, int support, float* y, void* stream);
int d4w_row_prefix_max_f32(const float* x, int nx, int ns, const double* mean, float* pmax, void* stream);
/* d4w_row_stats_f32 and d4w_row_prefix_max_f32 in one launch (the second sweep of a 60-s row is served by L2) */
int d4w_row_stats_prefix_f32(const float* x, int nx, int ns, double* mean, float* maxabs, float* pmax, void* stream);
int d4w_xcorr_dc_tail_rows_f32(const float* x, int nx, int ns, const double* mean, const float* maxabs,
                               double coef, int support, float* y, const float* pmax, float* rowmax, double eps,
                               void* stream);

/* Overlap-save FFT form of the same correlation for short templates (support <=
 * d4w_xcorr_fft_max_support() = 161 samples; the fin-whale templates have 136 / 156): blocks of
 * 4096 samples, one forward transform per block and one inverse per template, ~5x fewer flops than
 * the direct form, bound by HBM instead of the vector ALUs.  Same arguments and result as
 * d4w_xcorr_lens_f32 (agreement to float32 rounding); ws = DEVICE scratch of
 * d4w_xcorr_fft_ws_bytes() bytes (template spectra, rebuilt per call on `stream`). */
/* taps may be NULL in d4w_xcorr_fft_cont_f32 / d4w_fir_fft_f32 / d4w_fir_fft_halo_f32 when `ws` still holds the tables a
 * previous call on the same stream built from the same taps (same supports / half width): consecutive files of a record
 * then pay the template spectra once. */
int d4w_xcorr_fft_max_support(void);
size_t d4w_xcorr_fft_ws_bytes(void);
int d4w_xcorr_fft_f32(const float* x, int nx, int ns, const double* mean, const float* maxabs,
                      const float* taps, int ntpl, int ltaps, int len0, int len1, float* y0,
                      float* y1, void* ws, void* stream);
/* The same for a record that continues: lags whose window runs past sample ns - 1 read the first n_next samples of
 * xnext [nx][ld_next] (the head of the next file of the same cable, filtered the same way; de-meaned with THIS file's
 * row means like the row's own samples) instead of zeros -- what das4whales_amd/stream.py used to do by concatenating
 * the two files first (no reference counterpart, parity target = the reference run on the concatenated
 * record).  Two templates per call (the fused kernel).  xnext = NULL: identical to d4w_xcorr_fft_f32. */
int d4w_xcorr_fft_cont_f32(const float* x, int nx, int ns, const float* xnext, int ld_next, int n_next,
                           const double* mean, const float* maxabs, const float* taps, int ntpl, int ltaps,
                           int len0, int len1, float* y0, float* y1, void* ws, void* stream);

/* The same correlation as a banded-Toeplitz product on the matrix cores -- the form detect.compute_cross_correlogram
 * (detect.py:140-166) runs by default since round 4 (das4whales_amd/csrc/xcorr_mm.hip):
 *   C[i][a] = sum_u t[u - i] x[16 a + u]  per 256 lags, v_mfma_f32_16x16x32_f16 on binary16 hi / lo splits of the float32
 *   operands (three of the four partial products, float32 accumulation; agreement with d4w_xcorr_lens_f32 and a float64
 *   correlation to float32 rounding), one read of x and one write per correlogram, no workspace.
 * supports <= d4w_xcorr_mm_max_support() = 7936; ntpl = 1 or 2 (fused into one launch while both supports are <= 177; beyond,
 * one launch per template up to 497 taps -- the 450-sample template of scripts/main_mfdetect.py:70 --, and longer templates in
 * sections of 496 taps, each section one launch that reads x shifted by its first tap and accumulates into y); non-finite samples spread over the 256 lags of their tile in both templates.
 * mean / maxabs must be the rows' OWN statistics (|x - mean| / maxabs <= 2): with a continuation (xnext), whose head is scaled by
 * the row's statistics, and under D4W_MM_CLAMP=1 scaled samples beyond binary16's range are clamped to +-65504; elsewhere
 * statistics of another tensor can turn tiles into NaN (round 6: the clamp cost 2 % of the kernel on every call);
 * taps DEVICE [ntpl][ltaps], always needed (the
 * Toeplitz fragments are built in the kernel); mean / maxabs as d4w_xcorr_lens_f32 (maxabs == NULL: every 4096-lag chunk
 * is scaled by its own power of two); xnext / ld_next / n_next as d4w_xcorr_fft_cont_f32 (NULL, 0, 0: zeros behind the row). */
int d4w_xcorr_mm_max_support(void);
int d4w_xcorr_mm_f32(const float* x, int nx, int ns, const float* xnext, int ld_next, int n_next,
                     const double* mean, const float* maxabs, const float* taps, int ntpl, int ltaps,
                     int len0, int len1, float* y0, float* y1, void* stream);
/* The same, also leaving rowmax_t[c] = max_k y_t[c][k] (DEVICE float32 [nx] per template; rowmax1 only with ntpl = 2) from the
 * kernel's epilogue: what a detection threshold is set from (scripts/main_mfdetect.py:82,95: 0.5 * max of the correlograms)
 * without reading the correlograms again.  NULL, NULL: d4w_xcorr_mm_f32. */
int d4w_xcorr_mm_rowmax_f32(const float* x, int nx, int ns, const float* xnext, int ld_next, int n_next,
                            const double* mean, const float* maxabs, const float* taps, int ntpl, int ltaps,
                            int len0, int len1, float* y0, float* y1, float* rowmax0, float* rowmax1, void* stream);
/* The same, with the constant TAIL of the de-meaned zero-padded template added in the kernel's epilogue -- the whole of
 * detect.compute_cross_correlogram (detect.py:156-166: the template is normalised over its zero-padded length, detect.py:158, which
 * leaves -mean(t) / max|t| on the padding) in ONE pass over x, exact on every row:
 *   y_t[c][k] += tail_t * g[c] * sum_{i < k + len_t} (x[c][i] - m[c]),  k + len_t < ns;   tail_t = mean(t) / max|t| (0: no term).
 * (d4w_xcorr_dc_tail_rows_f32 adds the same term in a second pass over x and y, decided per row; this entry replaces the pair for
 * supports up to d4w_xcorr_mm_tail_max_support() = 497: one launch per template.)  Inside a block of 16 lags the term is part of
 * the Toeplitz product itself (the constant added to the staged taps); per block one prefix from a scan in the sample-conversion
 * phase; the prefix at a chunk's start carried along the row in float64 -- a workgroup walks whole rows (csrc/xcorr_mm.hip).
 * Needs mean and maxabs.  tail0 == tail1 == 0: d4w_xcorr_mm_rowmax_f32. */
int d4w_xcorr_mm_tail_max_support(void);
int d4w_xcorr_mm_tail_f32(const float* x, int nx, int ns, const float* xnext, int ld_next, int n_next,
                          const double* mean, const float* maxabs, const float* taps, int ntpl, int ltaps,
                          int len0, int len1, double tail0, double tail1, float* y0, float* y1,
                          float* rowmax0, float* rowmax1, void* stream);

/* Window-normalised matched filter (NMF, das4whales_amd/csrc/nmf.hip; no reference counterpart): a second pass that turns one
 * or two correlograms y_t of the rows of x -- produced by any d4w_xcorr_*_f32 with the SAME mean / maxabs (and the same
 * continuation), taps h'_t de-meaned over their support, no tail -- into correlation coefficients, in place:
 *   x'[i] = (x[c][i] - mean[c]) / maxabs[c] for i < ns, the same of xnext[c][i - ns] for ns <= i < ns + n_next, 0 beyond
 *   S1[k] = sum_{n < len_t} x'[k + n],  S2[k] = sum_{n < len_t} x'[k + n]^2,  V[k] = S2 - S1^2 / len_t (center = 1) or S2 (0)
 *   y_t[c][k] <- y_t[c][k] / (norm_t sqrt(V[k]))  where V[k] > floor^2 len_t,  0 elsewhere          (|.| <= 1 up to rounding)
 * norm_t = |h'_t|_2 from the host (0: a template without shape -- every lag 0); floor: the smallest window RMS, relative to
 * the row's max|x|, that is still divided by (dropouts, constant stretches and a one-tap window give 0, not rounding noise
 * over rounding noise); a row with maxabs = 0 gives zeros.  The windowed sums are float64 (sliding, re-anchored every 8 lags
 * from float64 sums of 8-sample runs), the final scale float32.  x is read once for both templates (len0 != len1 allowed),
 * every correlogram read and written once: 20 B per sample for a pair.  rowmax_t (DEVICE [nx], NULL or both with ntpl = 2):
 * max over the lags of the NORMALISED rows.  Supports <= d4w_nmf_max_support() = 7936 (>= d4w_xcorr_mm_max_support());
 * d4w_nmf_tile(): the lags one workgroup takes (what the tests size their row ends by).
 * Errors: D4W_EINVAL for a NULL x / y0 / mean / maxabs (y1 with ntpl = 2), nx or ns < 1, ntpl other than 1 or 2, a support
 * outside 1..d4w_nmf_max_support(), a norm or floor that is negative or not finite, center other than 0 / 1, n_next < 0 or
 * > ld_next, one rowmax of a pair without the other. */
int d4w_nmf_max_support(void);
int d4w_nmf_tile(void);
int d4w_nmf_normalise_f32(const float* x, int nx, int ns, const float* xnext, int ld_next, int n_next,
                          const double* mean, const float* maxabs, int ntpl, int len0, int len1,
                          double norm0, double norm1, int center, double floor, float* y0, float* y1,
                          float* rowmax0, float* rowmax1, void* stream);

/* STA/LTA energy detector and its on/off trigger (das4whales_amd/csrc/stalta.hip; no reference counterpart):
 * the template-free detector per channel.  With e[i] = x[c][i]^2 (the float32 sample widened to float64), samples before the
 * block at negative i:
 *   form 0, classic     STA[i] = (1/nsta) sum e[i-nsta+1 .. i],   LTA[i] = (1/nlta) sum e[i-gap-nlta+1 .. i-gap]
 *                       r[i] = STA / LTA  where both windows lie in known samples and LTA > (floor A)^2,  0 elsewhere
 *   form 1, recursive   sta[i] = sta[i-1] + (e[i] - sta[i-1]) / nsta, lta likewise with nlta (gap = 0), from rstate_in or 0
 *                       r[i] = sta / lta  where nseen + i + 1 >= nlta and lta > (floor A)^2,  0 elsewhere
 * A = scale[c] (DEVICE [nx]: the row's max|x| from d4w_row_stats_f32, or a per-channel noise level); a row with A = 0 (or NaN)
 * gives zeros.  Known samples: the block's own and the n_prev before it, prev = DEVICE [nx][ld_prev] whose columns
 * 0 .. n_prev - 1 are samples -n_prev .. -1 (classic form; the last max(nsta, nlta + gap) - 1 are all that is read).
 * rstate_in / rstate_out = DEVICE [nx][2] float64 (sta, lta) before / after the block (recursive form; NULL: zeros / not
 * wanted), nseen = samples of the record before the block.  x = DEVICE [nx][ld], ld in ELEMENTS (ld >= ns: a view is read in
 * place); ratio = DEVICE [nx][ld_r] or NULL.
 * Events (all of thr_on .. counts NULL: none): the trigger of d4w_trigger_onset_f32 runs on the ratios in registers; with
 * ratio == NULL nothing but the events is written (4 B per sample instead of 8 + 4).  Same arithmetic as the two calls in turn.
 * Numerics: every window sum is a float64 sum of parts of THAT window (samples, 8-sample runs, 64- and 512-sample blocks, all
 * non-negative): its error is relative to what the window holds and a window of zeros sums to 0.  The recursive form is a
 * float64 scan of (a, b) pairs.  One float64 division, rounded once to float32.  A NaN or Inf sample gives unspecified ratios
 * downstream of it.  Bytes: x read once, r written once; a tile's halo is read again from L2 by the workgroup that walks the row.
 * d4w_stalta_max_window() = 16384: the largest nlta + gap (and nsta); d4w_stalta_tile() = 2048: the samples of one anchor
 * period (one workgroup's tile; what the tests size their row ends by).
 * Errors: D4W_EINVAL for a NULL x or scale, nx or ns < 1, ld < ns, a form other than 0 / 1, nsta or nlta < 1, gap < 0, gap != 0
 * in the recursive form, nlta + gap or nsta > d4w_stalta_max_window(), a floor that is negative or not finite, n_prev < 0 or
 * > ld_prev or without prev, nseen < 0, neither ratio nor events asked for, ld_r < ns, some but not all of thr_on, thr_off, ev,
 * peak, counts, cap < 1. */
int d4w_stalta_max_window(void);
int d4w_stalta_tile(void);
int d4w_stalta_f32(const float* x, size_t ld, int nx, int ns, const float* prev, size_t ld_prev, int n_prev, int form,
                   int nsta, int nlta, int gap, double floor, const float* scale, const double* rstate_in,
                   double* rstate_out, long long nseen, float* ratio, size_t ld_r, const double* thr_on,
                   const double* thr_off, const int32_t* active_in, int32_t* active_out, int32_t* ev, float* peak,
                   int32_t* counts, int cap, void* stream);
/* Trigger events of the rows of r = DEVICE [nx][ld]: sample i is ON if r[i] > thr_on[c], OFF if r[i] < thr_off[c], KEEP
 * otherwise (a NaN is KEEP); the flag after sample i is the last ON / OFF at or before it, else active_in[c] (DEVICE int32 [nx],
 * NULL: inactive).  thr_on, thr_off = DEVICE [nx] float64, thr_off <= thr_on (not checked: they are on the device).  An event is
 * a maximal run of active samples: on = its first sample (-1: active on entry), off = one past its last (ns: still open),
 * peak index / peak = the position and value of the largest r of the run inside this block (the first on ties; -inf at the run's
 * first sample when it holds NaNs only).  Per row the first min(count, cap) events go to ev[c][cap][3] = (on, off, peak index)
 * and peak[c][cap], the true count to counts[c] (cap = ns / 2 + 1 always suffices; the caller repeats with a larger cap), the
 * flag after the last sample to active_out[c] (or NULL).  d4w_pick_offsets_i64(counts) and d4w_pack_events_i64 pack the rows into
 * out[4][total] int64 = (channel, on, off, peak index) and peak_out[total].
 * Errors: D4W_EINVAL for a NULL r / thr_on / thr_off / ev / peak / counts, nx or ns < 1, ld < ns, cap < 1 (pack: total < 0,
 * NULL out with total > 0). */
int d4w_trigger_onset_f32(const float* r, size_t ld, int nx, int ns, const double* thr_on, const double* thr_off,
                          const int32_t* active_in, int32_t* active_out, int32_t* ev, float* peak, int32_t* counts,
                          int cap, void* stream);
int d4w_pack_events_i64(const int32_t* ev, const float* peak, const int32_t* counts, const int64_t* offsets, int nx, int cap,
                        int64_t total, int64_t* out, float* peak_out, void* stream);

/* Local slant-stack semblance (das4whales_amd/csrc/semblance.hip; no reference counterpart): per channel and
 * sample the coherence of the 2M + 1 neighbouring channels along np trial moveouts, and the trial that maximises it.
 *   x = DEVICE [nx][pitch] float32, pitch in ELEMENTS (pitch >= ns: a column-sliced view is read in place).
 *   k, f = HOST [np][2M + 1]: the delay of trial j at neighbour m - M, split as floor(d) and float32(d - floor(d)) (a fraction
 *     that rounds to 1 carried into k); column M, the centre channel, is (0, 0).  w = HOST [2M + 1] weights >= 0, centre > 0.
 *   X(c, u) = x[c][u] for 0 <= u < ns, 0 elsewhere; a neighbour c + m outside [0, nx) or with w_m = 0 is absent.  Over the
 *   present neighbours in increasing m, float32, one fmaf per term:
 *     xi = v0 + f (v1 - v0), v0 = X(c + m, tau + k), v1 = X(c + m, tau + k + 1);  b = sum w xi, e = sum w xi^2, W = sum w
 *     N[t] = sum b^2, E[t] = sum e over tau in [max(0, t - H), min(ns - 1, t + H)];  S_j[c][t] = N / (W E) if W E > 0 else 0
 *   coh = DEVICE [nx][ns] float32 max_j S_j; idx = DEVICE [nx][ns] uint8, the smallest j attaining it; cube = DEVICE
 *   [np][nx][ns] float32 of every S_j, or NULL.  Window sums only ever add their non-negative terms in one fixed order (no
 *   running or prefix sums, no atomics): run-to-run bit-identical, and exact scaling of x by a power of two changes no bit.
 *   Non-finite input gives an unspecified result.  The table is uploaded in stream order for the call alone.
 * d4w_semblance_limits: the largest M (16), np (64), H (64) and |delay| in samples (64) a call takes.
 * d4w_semblance_tile: the output channels x samples one workgroup owns (what the tests size their shapes by).
 * Errors: D4W_EINVAL for a NULL required pointer, nx or ns < 1, pitch < ns, M, np or H outside the limits, a delay beyond
 *   +-64 samples, a fraction outside [0, 1), a non-zero centre delay, a weight that is negative or not finite, a centre
 *   weight of 0. */
int d4w_semblance_limits(int* max_half_aperture, int* max_slownesses, int* max_half_window, int* max_abs_delay);
int d4w_semblance_tile(int* channels, int* samples);
int d4w_semblance_f32(const float* x, int64_t pitch, int nx, int ns, const int32_t* k, const float* f, int np, int M,
                      const float* w, int H, float* coh, uint8_t* idx, float* cube /* or NULL */, void* stream);

/* Zero-phase FIR along time by overlap-save FFT blocks -- the INTERIOR of dsp.bp_filt / scipy.signal.sosfiltfilt
 * (dsp.py:859-880): away from the row ends a zero-phase IIR filter is the convolution with its two-sided response
 * g = h * h(-t), truncated at half width K where it has decayed below the tolerance (north star: "overlap-save FIR").
 *   y[r][n] = sum_{j <= 2K} taps[j] x[r][n - K + j]   for K <= n < ns - K;  the K columns at either row end are not
 *   written (the caller fills them with the exact recursion, d4w_sosfiltfilt_f32 on short pieces).
 * first[r] (device, e.g. the row's first sample) is subtracted before the transform and first[r] * dc_gain added
 * back, which keeps a large offset out of the float32 transform (dc_gain = |H(1)|^2 of the exact filter).
 * One read and one write of the block (8 B per sample).  K even, <= d4w_fir_fft_max_halfwidth(); ws as d4w_xcorr_fft_f32. */
int d4w_fir_fft_max_halfwidth(void);
int d4w_fir_fft_f32(const float* x, int nx, int ns, const float* taps, int K, const float* first, double dc_gain,
                    float* y, void* ws, void* stream);
/* The same filter writing only the output columns [col0, col1) (K <= col0 < col1 <= ns - K): the interior kernel of a band-pass
 * whose row-end columns are owned by d4w_sosfiltfilt_ends_f32 then touches none of them, and the two run side by side. */
int d4w_fir_fft_cols_f32(const float* x, int nx, int ns, const float* taps, int K, const float* first,
                         double dc_gain, float* y, int col0, int col1, void* ws, void* stream);
/* The same for a row that has neighbours on both sides (consecutive files of one record, das4whales_amd/stream.py):
 * left [nx][ld_left] holds the n_left samples before every row, right [nx][ld_right] the n_right samples after it
 * (n_left, n_right >= K), read in place -- no concatenated copy -- and ALL ns columns of y are written:
 *   y[r][n] = sum_j taps[j] xv[r][n - K + j],   xv = [left | x | right].
 * The row ends of a record (no neighbour) keep filtfilt's edge rule: d4w_sosfiltfilt_f32. */
int d4w_fir_fft_halo_f32(const float* x, int nx, int ns, const float* left, int ld_left, int n_left,
                         const float* right, int ld_right, int n_right, const float* taps, int K,
                         const float* first, double dc_gain, float* y, void* ws, void* stream);

/* ------------------------------------------------------------------------------------------
 * f-k mask design on the device (one-off per shape), float32 masks on the fftshift-ed (k, f)
 * grid, row-major [nx][ns] -- what d4w_fk_set_mask_dense_f32 takes.  Closed forms of the
 * reference's row / column loops; axis values in float64 as NumPy forms them.
 *   mode 0  dsp.fk_filter_design          dsp.py:85-171    params {cs_min, cp_min, cp_max, cs_max}
 *   mode 1  dsp.hybrid_filter_design      dsp.py:174-305   params {cs_min, cp_min, fmin, fmax}
 *   mode 2  dsp.hybrid_ninf_filter_design dsp.py:308-454   params {cs_min, cp_min, cp_max, cs_max};
 *           hrow_dev = DEVICE float64 [ns] band-pass row (zeros ++ |freqz(butter)|^2, dsp.py:348-349)
 *   mode 3  hybrid_gs_filter_design      before the blur (dsp.py:508-539)  params {-, cp_min, fmin, fmax}
 *   mode 4  hybrid_ninf_gs_filter_design before the blur (dsp.py:633-653)  params {-, cp_min, cp_max, -, fmin, fmax}
 *   mode 5  dsp.fk_filt wedge            before the blur (dsp.py:930-936)  params {c_min, c_max}
 * k_spacing = selected_channels[2]*dx (dsp.py:130), t_spacing = 1/fs; [i0, i1) = the half-open
 * column range the reference's loop runs over (np.argmax(f >= ...), host).
 * d4w_gaussian_filter_f32 = scipy.ndimage.gaussian_filter(., sigma) (truncate 4, reflect), used at
 * dsp.py:540,659,940; d4w_flip_sum_f32 = M + fliplr(M), then + flipud (dsp.py:660-661);
 * d4w_minmax_normalise_f32 = (g - min)/(max - min) in place (dsp.py:945), synchronises `stream`; a constant g
 * gives NaN everywhere like NumPy's 0 / 0.
 * ------------------------------------------------------------------------------------------ */
int d4w_design_mask_f32(int mode, int nx, int ns, double k_spacing, double t_spacing,
                        const double* params8_host, int i0, int i1, const double* hrow_dev,
                        float* mask, void* stream);
int d4w_flip_sum_f32(const float* in, float* out, int nx, int ns, void* stream);
int d4w_gaussian_filter_f32(const float* in, float* out, float* tmp, int nx, int ns, double sigma,
                            void* stream);
int d4w_minmax_normalise_f32(float* x, size_t n, void* stream);

/* ------------------------------------------------------------------------------------------
 * Row spectral operators (rows independent; every transform runs inside one workgroup's LDS).
 *
 * d4w_analytic_f32: scipy.signal.hilbert(x, axis=1) = ifft(fft(x) * h) per row, z = x + i H[x]
 *   mode 0  y = |z|                      envelope        (detect.py:192,217; scripts/main_mfdetect.py:58)
 *   mode 1  y = imag(z) = H[x]
 *   mode 2  y = 10 log10(|z|^2 / var[c]) var = DEVICE [nx] row variances   (dsp.py:975)
 *   mode 3  y[c][i] = diff(unwrap(angle z))[i] / (2 pi) * fs, [nx][ns-1]   (dsp.instant_freq, dsp.py:830-856)
 *   mode 4  y = |z| / sqrt(var[c])       improcess.trace2image before scaling   (improcess.py:60)
 *   Rows whose transform (ns / 2 packed values for even ns, ns for odd; the Bluestein convolution
 *   length when that has a prime factor > 31) fits one workgroup's LDS: d4w_analytic_row_fits_lds(ns);
 *   D4W_EINVAL otherwise -- those rows go through d4w_analytic_long_f32.
 * d4w_row_var_f32: var[c] = np.std(x[c])**2 (population).
 * d4w_snr_f32: dsp.snr_tr_array (dsp.py:956-976): 10 log10(x^2 / std^2) (env = 0) or the envelope
 *   form (env != 0); var_ws = DEVICE [nx] scratch.
 * d4w_fx_f32: dsp.get_fx (dsp.py:18-38): y[c][j] = 2 |fftshift(fft(x[c], nfft))|[j] / nfft * 1e9,
 *   y is [nx][nfft]; rows are cropped / zero-padded to nfft like np.fft.fft(x, nfft).
 * ------------------------------------------------------------------------------------------ */
int d4w_analytic_f32(const float* x, float* y, int nx, int ns, int mode, const float* var, double fs,
                     void* stream);
/* Rows too long for one workgroup's LDS (d4w_analytic_row_fits_lds(ns) == 0, e.g. 120 000 samples):
 * same modes through the four-step time-axis transform of the distributed f-k plan (two passes
 * each way over HBM) + the Hilbert pair op + one combine pass; any ns (odd ns: the rows as complex
 * sequences of their own length, scipy's one-sided multiplier on the spectrum; a prime factor > 31
 * of the transform length: the global-memory Bluestein form); ws = DEVICE scratch of
 * d4w_analytic_long_ws_bytes(nx, ns) bytes (4 nx ns for even ns, 8 nx ns for odd).  Shapes [nx][ns] with shape-specialised f-k kernels (built in or registered
 * through d4w_fk_register_shape) run that plan's time phase, its pass B with the Hilbert pair operation on real rows and
 * the inverse time phase instead (three fast passes + the combine pass; the ns / 2 prime-factor limit applies). */
int d4w_analytic_row_fits_lds(int ns);
size_t d4w_analytic_long_ws_bytes(int nx, int ns);
int d4w_analytic_long_f32(const float* x, float* y, int nx, int ns, int mode, const float* var, double fs,
                          void* ws, void* stream);
/* Frees the plans d4w_analytic_long_f32 keeps per (device, nx, ns) (it synchronises the device first; they are also dropped
 * once more than 16 shapes have been seen, so a stream of varying channel selections does not accumulate device tables). */
int d4w_analytic_long_clear(void);
int d4w_row_var_f32(const float* x, int nx, int ns, float* var, void* stream);
int d4w_snr_f32(const float* x, float* y, int nx, int ns, int env, float* var_ws, void* stream);
int d4w_fx_f32(const float* x, float* y, int nx, int ns, int nfft, void* stream);

/* ------------------------------------------------------------------------------------------
 * Welch power spectral density and energy of consecutive time chunks of every row: replaces the
 * per-chunk arithmetic of tools.spec / tools.__spec_chunk (tools.py:212-236) and
 * tools.energy_TimeDomain / tools._energy_TimeDomain_chunk (tools.py:84-157).  One read of x, no
 * workspace.
 *
 * d4w_welch_f32: for row c and chunk j < ns / chunk (a shorter remainder of the row is ignored)
 *     pxx[c][j][:] = scipy.signal.welch(x[c, j*chunk:(j+1)*chunk], fs=fs, nperseg=nperseg,
 *                                       noverlap=noverlap)[1]
 *   with SciPy's defaults: periodic Hann window, detrend='constant' (each segment's own mean, formed
 *   in float64, leaves the samples before the window), nfft = nperseg, segments every
 *   nperseg - noverlap samples while a whole one fits (d4w_welch_segments(chunk, nperseg, noverlap)
 *   of them), average='mean', scaling='density' = 1 / (fs sum(w^2)), one-sided with every bin but DC
 *   and Nyquist doubled.  pxx is DEVICE [nx][ns / chunk][d4w_welch_bins(nperseg) = nperseg/2 + 1].
 *   Accepted: nperseg even, 16 <= nperseg <= 4096, every prime factor of nperseg <= 31
 *   (d4w_welch_supported(nperseg) == 1), 0 <= noverlap < nperseg, nperseg <= chunk <= ns, fs > 0;
 *   D4W_EINVAL otherwise.
 * d4w_chunk_energy_f32: e[c][j] = sum(x[c, j*chunk : min((j+1)*chunk, ns)]**2), summed in float64;
 *   the last chunk may be short.  e is DEVICE [nx][ceil(ns / chunk)];  1 <= chunk <= ns.
 * ------------------------------------------------------------------------------------------ */
int d4w_welch_bins(int nperseg);
int d4w_welch_segments(int n, int nperseg, int noverlap);
int d4w_welch_supported(int nperseg);
int d4w_welch_f32(const float* x, int nx, int ns, int chunk, int nperseg, int noverlap, double fs,
                  float* pxx, void* stream);
int d4w_chunk_energy_f32(const float* x, int nx, int ns, int chunk, float* e, void* stream);

/* ------------------------------------------------------------------------------------------
 * Polyphase resampling and FIR decimation along time (csrc/resample.hip):
 * scipy.signal.resample_poly(x, up, down, axis=-1, window=h) and scipy.signal.decimate(x, q, ftype='fir') of every row,
 * for a file that does not arrive at the rate the chain works at.  up and down are reduced by their gcd; 1 / 1 is a copy.
 * With h = the ntaps taps (float32, DEVICE; the caller has multiplied them by up), half = (ntaps - 1) / 2 and
 * n_out = d4w_resample_out_len(ns, up, down) = ceil(ns up / down):
 *
 *     y[r][m] = back_r + scale * sum_i (xv[r][i] - off_r) h[m down + half - i up],     m < n_out
 *
 * over all i with 0 <= m down + half - i up < ntaps for which xv[r][i] exists: xv is x[r][i] for 0 <= i < ns,
 * left[r][n_left + i] for -n_left <= i < 0 and right[r][i - ns] for ns <= i < ns + n_right.  A sample that does not
 * exist contributes nothing: the zero padding follows the removal of the offset.  With off = 0, scale = 1 and no
 * neighbours this is resample_poly(padtype='constant') term for term.  Every output is summed by one thread in ascending
 * tap order: the result is the same bits run to run and wherever a row is cut into blocks with neighbours.
 *
 * d4w_resample_f32: x is [nx] rows of ns float32, ld_x apart; left / right (may be NULL) hold the n_left samples before and
 *   the n_right samples after every row, rows ld_left / ld_right apart, read in place; they need ns up % down == 0 after
 *   the reduction (the output grids of consecutive blocks line up).  off_r = off[r] (DEVICE float64, e.g. the means of
 *   d4w_row_stats_f32) or off_const when off == NULL; it leaves a sample as (x - hi) - lo, hi + lo its two-float form.
 *   add_back = 0: back_r = 0;  1: back_r = off_r (padtype='mean': the offset is put back as it was);  2: back_r =
 *   scale off_r sum_j h[t + j up] over the taps t of the output's phase -- the record continues as the constant off_r
 *   beyond its ends (SciPy's padtype='constant' with cval; the taps of a phase sum to 1 only within ~1e-3 for up > 1).
 *   y: float32 [nx][n_out].
 * d4w_resample_raw_f32: the same kernel reading the raw rows c0 + r cstep, r < nx_out, of a [nch][ns] matrix
 *   (raw_dtype as d4w_raw2strain_f32) -- the fused ingest: off_r = mean[r] (d4w_raw_row_mean_f64) is removed in float64
 *   before the sample is rounded to float32, scale = the file's scale factor, nothing is added back, no neighbours.
 * d4w_raw_row_mean_f64: mean[r] of those raw rows as float64; integer rows are summed as integers (exact).
 * d4w_resample_reach: the neighbour samples the taps reach before sample 0 and after sample ns - 1 of a block whose
 *   ns up is a multiple of down.
 * Limits (D4W_EINVAL beyond them; there is no other path): 1 <= ntaps <= d4w_resample_max_taps() = 2048 (designed
 * taps up to max(up, down) = 102), up and down <= 256 after the reduction.
 * ------------------------------------------------------------------------------------------ */
int d4w_resample_max_taps(void);
int d4w_resample_out_len(int ns, int up, int down);
int d4w_resample_reach(int ntaps, int up, int down, int* n_left, int* n_right);
int d4w_resample_f32(const float* x, size_t ld_x, int nx, int ns, const float* left, size_t ld_left, int n_left,
                     const float* right, size_t ld_right, int n_right, const float* taps, int ntaps, int up, int down,
                     const double* off, double off_const, double scale, int add_back, float* y, void* stream);
int d4w_resample_raw_f32(const void* raw, int raw_dtype, int ns, int c0, int cstep, int nx_out, const float* taps,
                         int ntaps, int up, int down, const double* mean, double scale, float* y, void* stream);
int d4w_raw_row_mean_f64(const void* raw, int raw_dtype, int ns, int c0, int cstep, int nx_out, double* mean,
                         void* stream);

/* ------------------------------------------------------------------------------------------
 * Spectrograms and spectrogram correlation: replaces dsp.get_spectrogram (dsp.py:41-78),
 * detect.get_sliced_nspectrogram (detect.py:334-408), detect.xcorr2d (detect.py:579-602),
 * detect.xcorr (detect.py:605-647) and the per-channel loop of
 * detect.compute_cross_correlogram_spectrocorr (detect.py:650-709).
 *
 * d4w_stft_mag_f32: S[c][b - bin_lo][t] = |librosa.stft(x[c], n_fft, hop_length=hop)|[b][t] for
 *   bin_lo <= b <= bin_hi, t < d4w_stft_frames(ns, hop) = 1 + ns/hop (periodic Hann, center=True
 *   with zero padding: librosa >= 0.10 defaults).  rowmax[c] = max over ALL bins and frames (what
 *   detect.py:387 / dsp.py:76 normalise by).  n_fft even, <= 6144; a window with a prime factor > 31 runs its frame
 *   transform as a Bluestein convolution.  rowmax may be NULL for n_fft = 128, 160, 256, 512
 *   (two-factor register transforms): then only the kept bins are formed (detect.compute_cross_correlogram_spectrocorr,
 *   where the normalisation cancels against the median).
 * d4w_scale_rows_f32: S[c][:] /= denom[c] (mode 0) or 20 log10(S[c][:] / denom[c]) (mode 1).
 * d4w_row_median_f32: med[c] = np.median(v[c][0:per_row]).
 * d4w_spectrocorr_f32:
 *   raw[c][t] = sum_f sum_j S[c][f][t + j - off] K[f][j]  (zero outside the spectrogram), t < nout
 *   zero_ends == 0: out[c][t] = max(raw, 0) / (med[c] * nk)  (clipped, then divided: detect.py:599-600);
 *   zero_ends != 0: out[c][t] = max(raw / (med[c] * nk), 0) with out[c][0] = out[c][nout-1] = 0  (divided, then
 *   clipped: detect.py:642-645).  The forms differ only for med[c] < 0.  An all-zero row gives NaN (0 / 0) in both.
 *   off = nk/2, nout = nt, zero_ends = 0: detect.xcorr2d;  off = 0, nout = nt-nk+1, zero_ends = 1: detect.xcorr.
 *   S [nx][nf][nt], K [nf][nk], med [nx], out [nx][nout], all DEVICE float32.
 * ------------------------------------------------------------------------------------------ */
int d4w_stft_frames(int ns, int hop);
int d4w_stft_mag_f32(const float* x, float* S, float* rowmax, int nx, int ns, int n_fft, int hop,
                     int bin_lo, int bin_hi, void* stream);
/* The same magnitudes for the detector's call shape -- a few kept bins of a heavily overlapped transform, no row maximum
 * (detect.compute_cross_correlogram_spectrocorr, detect.py:650-709: n_fft = 160, hop = 8, the 13 bins between 14 and 30 Hz) --
 * as ONE matrix product per 16 frames on the matrix cores: X[b][t] = sum_u (w[u] e^{-2 pi i b u / N}) x[hop t - N/2 + u],
 * operands as binary16 hi / lo pairs with float32 accumulation (das4whales_amd/csrc/stft_mm.hip).  d4w_stft_mag_f32 takes this
 * route by itself when rowmax == NULL and d4w_stft_mm_eligible(...) = 1: n_fft % 32 == 0 <= 160, hop % 8 == 0 <= 32, at most
 * 16 kept bins (D4W_STFT_MM=0 switches it off). */
int d4w_stft_mm_eligible(int n_fft, int hop, int bin_lo, int bin_hi);
int d4w_stft_mag_mm_f32(const float* x, float* S, int nx, int ns, int n_fft, int hop, int bin_lo, int bin_hi,
                        void* stream);
int d4w_scale_rows_f32(float* S, int nx, size_t per_row, const float* denom, int mode, void* stream);
int d4w_row_median_f32(const float* v, int nx, size_t per_row, float* med, void* stream);
int d4w_spectrocorr_f32(const float* S, int nx, int nf, int nt, const float* K, int nk, int off,
                        int nout, const float* med, int zero_ends, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Exact order statistics of every row: out[c][j] = np.quantile(v[c][0:per_row].astype(float64), q[j]) with NumPy's default
 * "linear" method, rounded once to float32 -- the per-channel median of scripts/main_bathynoise.py:139 and any other quantile
 * of a row.  With h = q (n - 1): the order statistics of ranks floor(h) and floor(h) + 1 (the last one twice at q = 1), exact,
 * by a radix select on order-preserving keys (no sort, no sample), interpolated in float64 by NumPy's own formula -- so a row
 * with infinities gives what NumPy gives, a NaN where NumPy's a + (b - a) g meets inf - inf or inf * 0.
 *   v: DEVICE, rows `ld` elements apart (a column window of a block is read in place); q_host: HOST [nq], 0 <= q <= 1;
 *   nq in 1 .. d4w_row_quantile_limits (8).  A row that holds a NaN gives NaN for every q; -0 and +0 are equal.
 * All nq quantiles come out of one launch: one sweep of the row shared by all of them, two more per quantile.
 * ------------------------------------------------------------------------------------------ */
int d4w_row_quantile_f32(const float* v, int nx, size_t per_row, size_t ld, const double* q_host, int nq,
                         float* out, void* stream);
int d4w_row_quantile_limits(int* max_q);

/* ------------------------------------------------------------------------------------------
 * The noise floor of every channel (scripts/main_bathynoise.py): per row c of x [nx][ns] (rows `ld` elements apart: a time
 * window of a block is read in place, and the Hilbert transform is that of the window, main_bathynoise.py:256-259)
 *   mean_sq[c]  = np.mean(x**2)                               main_bathynoise.py:257
 *   std[c]      = np.std(x)  (population)                     main_bathynoise.py:189
 *   env_mean[c] = np.mean(abs(scipy.signal.hilbert(x)))       main_bathynoise.py:186,259
 *   env_q[c][j] = np.quantile(abs(hilbert(x)), q[j])          main_bathynoise.py:139,183 (q = 0.5), d4w_row_quantile_f32's definition
 * The envelope is d4w_analytic_f32's mode 0.  Every output pointer may be NULL; nq = 0 .. 8 (env_q NULL with nq = 0); sums in
 * float64 in an order that depends on ns and the form alone (bit-identical run to run, whatever nx and the other rows).
 *   how = 1  one-read form, rows with d4w_channel_noise_fits_lds(ns) = 1: one workgroup per row transforms it in LDS, keeps
 *            the envelope there and selects from LDS -- one read of the block, nx (3 + nq) floats written; ws is not used.
 *   how = 2  long-row form, any ns: envelope by d4w_analytic_long_f32 into ws (DEVICE, d4w_channel_noise_ws_bytes(nx, ns)),
 *            then the select and a moment sweep over global memory; nx > 65535 in slabs.
 *   how = 0  the one-read form where it fits, else the long-row form.
 * ------------------------------------------------------------------------------------------ */
int d4w_channel_noise_fits_lds(int ns);
size_t d4w_channel_noise_ws_bytes(int nx, int ns);
int d4w_channel_noise_f32(const float* x, int nx, int ns, size_t ld, const double* q_host, int nq,
                          float* mean_sq, float* std, float* env_mean, float* env_q, void* ws, int how, void* stream);

/* ------------------------------------------------------------------------------------------
 * Peak picking: scipy.signal.find_peaks(x[c], prominence=thr)[0] per row, replaces the loops of
 * detect.pick_times / pick_times_env / process_corr / pick_times_par (detect.py:169-274; the
 * envelope of the *_env variants is d4w_analytic_f32 mode 0).  Strict local maxima with plateaus
 * reported at their middle sample, prominence with wlen=None, kept when prominence >= thr
 * (compared in float64, as SciPy does on the float64 view of the same samples).
 *   idx [nx][cap] int32: the first min(counts[c], cap) peak positions of row c in time order;
 *   counts[c] = number of peaks found (may exceed cap: call again with a larger cap; ns/2 always suffices).
 * ------------------------------------------------------------------------------------------ */
int d4w_find_peaks_f32(const float* x, int nx, int ns, double prominence, int32_t* idx,
                       int32_t* counts, int cap, void* stream);
/* The same with the threshold formed on the device: prominence = scale * value[0] (float64 product of the float32 DEVICE
 * scalar, exactly the host's 0.45 * float(np.max(corr)) of scripts/main_mfdetect.py:82,95) -- a chain that takes its
 * threshold from the block's largest correlation (d4w_minmax_f32, d4w_xcorr_mm_rowmax_f32) need not wait for it. */
int d4w_find_peaks_dthr_f32(const float* x, int nx, int ns, const float* value, double scale, int32_t* idx,
                            int32_t* counts, int cap, void* stream);
/* One threshold per row: prominence of row c = scale * (double)thr[c], thr DEVICE [nx] -- "k times this channel's noise floor"
 * (the per-channel median envelope of scripts/main_bathynoise.py:139,183 from d4w_channel_noise_f32).  As in SciPy a NaN or
 * +inf bar yields no pick in its row and a zero or negative bar every strict local maximum. */
int d4w_find_peaks_rowthr_f32(const float* x, int nx, int ns, const float* thr, double scale, int32_t* idx,
                              int32_t* counts, int cap, void* stream);
/* offsets[c] = counts[0] + ... + counts[c] (int64, what d4w_pack_picks_i64 places the rows by) and
 * summary2 = {max_c counts[c], sum_c counts[c]} (DEVICE int64[2]: the capacity check and the table size of one picker call). */
int d4w_pick_offsets_i64(const int32_t* counts, int nx, int64_t* offsets, int64_t* summary2, void* stream);
/* The picks of all rows as one packed table out[2][total] int64, row 0 = channel index, row 1 = time index
 * -- what detect.convert_pick_times builds from the ragged lists (detect.py:277-303; the reference's docstring
 * has the two rows swapped, :289 vs :297-299).  offsets[c] = counts[0] + ... + counts[c] (inclusive prefix sum,
 * device), total = offsets[nx - 1]; every counts[c] must be <= cap. */
int d4w_pack_picks_i64(const int32_t* idx, const int32_t* counts, const int64_t* offsets, int nx, int cap,
                       int64_t total, int64_t* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Image operators of the Gabor detector: replaces improcess.scale_pixels /
 * trace2image (improcess.py:23-62), improcess.binning (improcess.py:395-420, torchvision Resize =
 * antialiased bilinear interpolation), cv2.filter2D and the thresholds of
 * scripts/main_gabordetect.py:109-134, improcess.apply_smooth_mask (improcess.py:423-454).
 * Images are row-major float32 [h][w] on the DEVICE.
 *
 * d4w_minmax_f32: minmax[0] = min(x), minmax[1] = max(x) over n values; minmax = DEVICE [2].
 * d4w_scale_pixels_f32: y = (x - minmax[0]) / (minmax[1] - minmax[0]) * gain; y may alias x.
 * d4w_threshold_f32: y = (x > thr) ? 1 : 0, compared in float64.
 * d4w_mask_mul_f32: y = x where mask != 0, else 0 (array * bool mask).
 * d4w_resize_bilinear_aa_f32: torch.nn.functional.interpolate(x, (oh, ow), mode="bilinear",
 *   align_corners=False, antialias=True) -- what torchvision 0.17 Resize runs; horizontal pass, then
 *   vertical pass; ws = DEVICE scratch of d4w_resize_ws_bytes(h, w, oh, ow) bytes.
 * d4w_filter2d_f32: cv2.filter2D(img, CV_64F, kernel): out[y][x] = sum K[ky][kx] *
 *   img[y + ky - kh/2][x + kx - kw/2] with BORDER_REFLECT_101; kernel = DEVICE [kh][kw];
 *   accumulate != 0 adds to out; ws = DEVICE scratch of d4w_filter2d_ws_bytes(kh, kw) bytes.
 *   (64 + kw - 1)(32 + kh - 1) floats must fit in 160 KiB of LDS (101 x 101: 85 KiB).
 * ------------------------------------------------------------------------------------------ */
int d4w_minmax_f32(const float* x, size_t n, float* minmax, void* stream);
int d4w_scale_pixels_f32(const float* x, float* y, size_t n, const float* minmax, double gain, void* stream);
int d4w_threshold_f32(const float* x, float* y, size_t n, double thr, void* stream);
int d4w_mask_mul_f32(const float* x, const float* mask, float* y, size_t n, void* stream);
size_t d4w_resize_ws_bytes(int h, int w, int oh, int ow);
int d4w_resize_bilinear_aa_f32(const float* x, int h, int w, float* y, int oh, int ow, void* ws, void* stream);
size_t d4w_filter2d_ws_bytes(int kh, int kw);
int d4w_filter2d_f32(const float* img, int h, int w, const float* kernel, int kh, int kw, float* out,
                     int accumulate, void* ws, void* stream);
/* The same correlation on the matrix cores for kernels of <= 113 columns (the detector's 101 x 101 Gabor kernels): kernel row
 * by kernel row a banded-Toeplitz product, out[y][16 a + i] += sum_u K[j][u - i] P[y + j][16 a + u], operands as binary16
 * hi / lo pairs with float32 accumulation (das4whales_amd/csrc/filter2d_mm.hip).  d4w_filter2d_f32 takes this route by itself
 * when d4w_filter2d_mm_eligible(kh, kw) = 1 (D4W_F2D_MM=0 switches it off); ws of the stand-alone entry point: DEVICE scratch of
 * d4w_filter2d_mm_ws_bytes(kh, kw) bytes. */
int d4w_filter2d_mm_eligible(int kh, int kw);
size_t d4w_filter2d_mm_ws_bytes(int kh, int kw);
int d4w_filter2d_mm_f32(const float* img, int h, int w, const float* kernel, int kh, int kw, float* out,
                        int accumulate, void* ws, void* stream);

/* ------------------------------------------------------------------------------------------
 * Radon transform: replaces improcess.compute_radon_transform (improcess.py:347-367), i.e.
 * skimage.transform.radon(image, theta, circle=False) (das4whales_amd/csrc/radon.hip).
 *
 * d4w_radon_size: P = ceil(sqrt(2) max(h, w)), the side of the zero-padded square and the number of
 *   sinogram rows; -1 for an empty image.
 * d4w_radon_f32: out[c][i] = sum_r bilinear(img padded to P x P, y, x) with, for a = theta_deg[i] in radians and
 *   c0 = P / 2, x = cos a c + sin a r - c0 (cos a + sin a - 1), y = -sin a c + cos a r - c0 (cos a - sin a - 1);
 *   pad_before = P / 2 - {h, w} / 2, zeros outside the image.  img = DEVICE [h][w], out = DEVICE [P][ntheta],
 *   theta_deg = HOST [ntheta] degrees (finite, any range); ntheta = 0 writes nothing.  ws = DEVICE scratch of
 *   d4w_radon_ws_bytes(h, w, ntheta) bytes (the per-angle cos / sin table).  Run-to-run bit-identical.
 * ------------------------------------------------------------------------------------------ */
int d4w_radon_size(int h, int w);
size_t d4w_radon_ws_bytes(int h, int w, int ntheta);
int d4w_radon_f32(const float* img, int h, int w, const double* theta_deg_host, int ntheta, float* out, void* ws,
                  void* stream);

/* ------------------------------------------------------------------------------------------
 * Edge stencils, Gaussian blur and bilateral filter (das4whales_amd/csrc/edges.hip): the image operators of
 * improcess.py outside the Gabor detector.  Images are row-major float32 [h][w] on the DEVICE, out must not alias img,
 * h w <= INT32_MAX.  Every output element is written by one thread in a fixed order: run-to-run bit-identical.
 *
 * d4w_stencil_zero_f32: out[y][x] = sum_ij kernel[i][j] img[y + i - anchor_y][x + j - anchor_x] with ZEROS outside the
 *   image (d4w_filter2d_f32 reflects); kernel = HOST float64 [kh][kw], kh, kw <= 7, anchor inside the kernel.  Replaces the
 *   two scipy.signal.fftconvolve(mode='same') calls of improcess.detect_diagonal_edges (improcess.py:172-226; pass the
 *   summed kernel flipped in both axes, anchor = centre) and the two conv2d(padding=1) calls of
 *   improcess.diagonal_edge_detection (improcess.py:229-266; the summed 3 x 3 kernel, anchor (1, 1)).
 * d4w_gradient_oriented_f32: improcess.gradient_oriented (improcess.py:143-169), direction = (dft, dfx) >= 0:
 *   dfx = 0: out[h][w - dft]         = -(img[y][x] - img[y][x + dft])
 *   dft = 0: out[h - dfx][w]         = -(img[y + dfx][x] - img[y][x])
 *   else:    out[h - 2 dfx][w - dft] = -(img[y + dfx][x] - 0.5 img[y + 2 dfx][x + dft] - 0.5 img[y][x + dft])
 *   (0, 0) and shifts that leave no output write nothing (out may then be NULL).
 * d4w_gaussian_blur_f32: cv2.GaussianBlur's arithmetic for float images (improcess.gaussian_filter, improcess.py:370-392):
 *   out = columns(taps_y) of rows(taps_x) of img, correlation with the anchor at the centre, BORDER_REFLECT_101 (repeated
 *   for images smaller than the kernel).  taps = HOST float64, odd lengths ky, kx; the caller computes them (OpenCV's
 *   getGaussianKernel).  ky, kx <= 31: one launch, ws unused (d4w_gaussian_blur_ws_bytes = 0, ws may be NULL); larger: two
 *   launches through ws = DEVICE scratch of d4w_gaussian_blur_ws_bytes(h, w, ky, kx) bytes.  NOT d4w_gaussian_filter_f32,
 *   which is scipy.ndimage.gaussian_filter of the mask designers.
 * d4w_bilateral_f32: cv2.bilateralFilter by its documented definition (improcess.bilateral_filter, improcess.py:319-344):
 *   out(p) = sum_q w I(q) / sum_q w over the offsets of the (2 radius + 1)^2 square, BORDER_REFLECT_101,
 *   w = space_w[q - p] exp(-(I(q) - I(p))^2 / (2 sigma_color^2)); space_w = DEVICE float32 [(2 radius + 1)^2], the
 *   caller's spatial weights, 0 at the offsets outside the circle (skipped); sigma_color > 0.  radius <=
 *   d4w_bilateral_max_tiled_radius() (15) runs from an LDS tile, larger radii (<= 1024) from global memory.
 * ------------------------------------------------------------------------------------------ */
int d4w_stencil_zero_f32(const float* img, int h, int w, const double* kernel_host, int kh, int kw, int anchor_y,
                         int anchor_x, float* out, void* stream);
int d4w_gradient_oriented_f32(const float* img, int h, int w, int dft, int dfx, float* out, void* stream);
size_t d4w_gaussian_blur_ws_bytes(int h, int w, int ky, int kx);
int d4w_gaussian_blur_f32(const float* img, int h, int w, const double* taps_y_host, const double* taps_x_host, int ky,
                          int kx, float* out, void* ws, void* stream);
int d4w_bilateral_max_tiled_radius(void);
int d4w_bilateral_f32(const float* img, int h, int w, int radius, const float* space_w, double sigma_color, float* out,
                      void* stream);

/* ------------------------------------------------------------------------------------------
 * Least-squares localisation (das4whales_amd/csrc/loc.hip): the reference's loc.py, batched.  float64 throughout; every
 * pointer is DEVICE memory unless marked otherwise; cable_pos = [nch][3] (x, y, z in metres), Ti = [ncalls][nch] arrival
 * times in seconds where NaN means "no pick on this channel"; c0 > 0.  Every output element is written by one thread and
 * every sum has a fixed order: run-to-run bit-identical.
 *
 * d4w_loc_solve_f64: loc.solve_lq (loc.py:57-128) for ncalls calls at once, one workgroup per call.  Nbiter damped
 *   Gauss-Newton steps on n = [x, y, z, t0] (z held with fix_z): rows of G = cos th cos ph / c0, cos th sin ph / c0,
 *   sin th / c0 (absent with fix_z), 1 with th = atan2(|z_w - z_c|, r), ph = atan2(y_w - y_c, x_w - x_c);
 *   dn = (G^T G + 1e-5 I)^-1 G^T (Ti - t0 - R / c0); n += 0.7 dn in the first four iterations, n += dn after.
 *   first_guess = [ncalls][4], or NULL for the reference's [40000, 23000, -60, min of the call's valid Ti] (loc.py:86).
 *   history [ncalls][Nbiter][4] = n after every iteration (may be NULL when Nbiter = 0), n_out [ncalls][4] = the last one.
 *   At n_out, over the channels that carry a pick: gtg [ncalls][p][p] = G^T G without the regularisation (p = 3 with fix_z,
 *   else 4) -- the matrix loc.calc_covariance_matrix (loc.py:156-191) rebuilds --, ssr [ncalls] = the sum of squared
 *   residuals (loc.cal_variance_residuals, loc.py:131-153, divides it by npick - p) and npick [ncalls] (int32).  Nbiter = 0
 *   evaluates these at first_guess.  A call without a pick gives NaN rows in history and n_out, zeros elsewhere.
 * d4w_loc_misfit_grid_f64: for every call and every node (xs[ix], ys[iy], z) of a grid, the best emission time
 *   t0 = mean over the picked channels of e = Ti - |cable - node| / c0 and rms = sqrt(mean (e - t0)^2).
 *   rms, t0 = [ncalls][ny][nx]; NaN for a call without a pick.  ncalls <= 65535.
 * d4w_loc_arrival_times_f64: loc.calc_arrival_times (loc.py:13-25) for npos positions at once:
 *   out [npos][nch] = t0[p] + |cable - pos[p]| / c0, pos = [npos][3], t0 = [npos].  npos <= 65535.
 * ------------------------------------------------------------------------------------------ */
int d4w_loc_solve_f64(const double* cable_pos, int nch, const double* Ti, int ncalls, double c0, int nbiter, int fix_z,
                      const double* first_guess, double* history, double* n_out, double* gtg, double* ssr, int* npick,
                      void* stream);
int d4w_loc_misfit_grid_f64(const double* cable_pos, int nch, const double* Ti, int ncalls, double c0, const double* xs, int nx,
                            const double* ys, int ny, double z, double* rms, double* t0, void* stream);
int d4w_loc_arrival_times_f64(const double* cable_pos, int nch, const double* pos, const double* t0, int npos, double c0,
                              double* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Association of picks into calls (das4whales_amd/csrc/assoc.hip): a delay-and-vote over a position grid, the step
 * between detect.pick_times* and the localisation above (the reference has none).  float64 arithmetic, int32 votes; every
 * pointer is DEVICE memory.  Votes are integers, so every result is run-to-run bit-identical.
 *
 *   picks [2][npicks] int64: row 0 = channel ch_k (0 <= ch_k < nch), row 1 = sample i_k, ordered by (channel, sample) --
 *     the packed table of d4w_pack_picks_i64; t_k = i_k / fs.  npicks <= 2^30; npicks = 0 is valid (picks may be NULL).
 *   node g = iy nx + ix at (xs[ix], ys[iy], z), the layout of d4w_loc_misfit_grid_f64.
 *   e_kg = t_k - |cable_pos[ch_k] - node_g| / c0                  emission time of pick k if it came from node g
 *   bin(k, g) = floor((e_kg - lo) / dt)                           (evaluated as (e_kg - lo) * (1 / dt), |..| * (1 / c0))
 *   votes[g][b] = #{k : bin(k, g) = b}, 0 <= b < nbins            picks whose bin falls outside are not counted
 *   s[g][b] = votes[g][b] + votes[g][b + 1], 0 <= b < nbins - 1   a call astride a bin edge is not split
 *
 * d4w_assoc_vote_i32: votes [ny nx][nbins] = sign * count (accumulate = 0) or += sign * count (accumulate != 0), counted over
 *   all picks (idx = NULL) or over the picks idx[0 .. nidx - 1] (int32 positions in the table, entries < 0 are skipped:
 *   the `chosen` list of d4w_assoc_select_f64, read in place).  sign = +1 or -1.  stop = NULL, or a DEVICE int32 that makes
 *   the launch return at once when non-zero (state of d4w_assoc_best_i32).  No global atomics: every element of votes is
 *   written by one workgroup.  nbins above the 1024-bin LDS tile runs one pass over the picks per 1024 bins.
 * d4w_assoc_best_i32: (g*, b*) = arg-max of s, ties to the smallest flat index g (nbins - 1) + b.  state = int32 [2] =
 *   {stop, calls found}, zeroed by the caller before the first round.  If state[0] != 0 nothing happens.  If
 *   s[g*][b*] < min_picks: state[0] = 1.  Else rec[call][0 .. 3] = {g*, b*, s[g*][b*], 0} and state[1] = call + 1.
 *   rec = int32 [calls][4]; ws = DEVICE scratch of d4w_assoc_best_ws_bytes() bytes.
 * d4w_assoc_select_f64: for round `call` (nothing happens if state[0] != 0), with (g*, b*) = rec[call][0 .. 1] and the window
 *   centre ec = lo + (b* + 1) dt: per channel, among its picks k with assigned[k] = 0 and bin(k, g*) in {b*, b* + 1}, the one
 *   of smallest |e_kg* - ec|, ties to the smaller k.  offsets [nch] int64 = inclusive prefix sum of the picks per channel
 *   (d4w_pick_offsets_i64): channel c owns picks offsets[c - 1] .. offsets[c] - 1.  Writes Ti[call][c] = t_k (NaN: none),
 *   chosen[c] = k (-1: none), e_chosen[c] = e_kg* (NaN: none), assigned[k] = call + 1; then rec[call][3] = channels chosen
 *   and first_guess[call] = {xs[ix*], ys[iy*], z, mean of e_chosen over the chosen channels} (the form d4w_loc_solve_f64
 *   takes).  Ti = [calls][nch], chosen = int32 [nch], e_chosen = [nch], assigned = int32 [npicks], first_guess = [calls][4].
 *
 * One greedy round is best, select, vote(idx = chosen, sign = -1, accumulate = 1, stop = state): afterwards votes is the vote
 * of the picks with assigned = 0 counted from scratch.  All rounds can be enqueued without a host synchronisation; state[1]
 * is then the number of calls.
 * Errors: D4W_EINVAL for nch < 1, nx < 1, ny < 1, nbins < 2, dt, fs or c0 not finite or <= 0, sign other than +1 / -1,
 *   a NULL required pointer, npicks or call < 0.
 * ------------------------------------------------------------------------------------------ */
int d4w_assoc_vote_i32(const int64_t* picks, int npicks, const int32_t* idx, int nidx, int sign, int accumulate,
                       const double* cable_pos, int nch, double fs, double c0, const double* xs, int nx, const double* ys, int ny,
                       double z, double lo, double dt, int nbins, int32_t* votes, const int32_t* stop, void* stream);
size_t d4w_assoc_best_ws_bytes(void);
int d4w_assoc_best_i32(const int32_t* votes, int nx, int ny, int nbins, int min_picks, int call, int32_t* state, int32_t* rec,
                       void* ws, void* stream);
int d4w_assoc_select_f64(const int64_t* picks, int npicks, const int64_t* offsets, const double* cable_pos, int nch, double fs,
                         double c0, const double* xs, int nx, const double* ys, int ny, double z, double lo, double dt, int nbins,
                         int call, const int32_t* state, int32_t* rec, int32_t* assigned, double* Ti, int32_t* chosen,
                         double* e_chosen, double* first_guess, void* stream);

/* ------------------------------------------------------------------------------------------
 * Delay-and-sum stack of envelopes over the position grid (das4whales_amd/csrc/stack.hip): the soft-decision twin of the
 * vote above -- no per-channel threshold comes before the sum over the channels (the reference has none of this).  Every
 * pointer is DEVICE memory.  Layouts as above: cable_pos [nch][3] float64, node g = iy nx + ix at (xs[ix], ys[iy], z).
 *
 *   env [nch][ns] float32 with a row pitch in ELEMENTS (pitch >= ns: a column-sliced view is read in place), the envelope of
 *     a correlogram; weights [nch] float32, or NULL for ones.
 *   d[g][ch] = (int) floor(|cable_pos[ch] - node_g| * (1 / c0) * fs + 0.5)        travel time in samples, float64, capped
 *     at 2^30; csrc/moveout.h is the single definition of the distance and the delay for the vote, this stack and the beam
 *     below: differences first, one square root, 1 / c0 formed once on the host, no contraction.
 *   stack[g][k - k0] = sum over ch, in increasing ch, of weights[ch] * env[ch][k + d[g][ch]]             k0 <= k < k1
 *     over the channels with weights[ch] != 0 and 0 <= k + d[g][ch] < ns
 *
 * d4w_stack_delays_i32: delays [ny nx][nch] int32 = d.  One thread per element.
 * d4w_stack_grid_f32: stack [ny nx][k1 - k0] float32 from env and a delay table (d4w_stack_delays_i32's; kept by the caller
 *   across the files of one geometry).  Columns are emission samples k0 .. k1 - 1; k0 may be negative and k1 may exceed ns
 *   (-2^30 <= k0 < k1 <= 2^30, k1 - k0 <= 2^31 - 1).  float32 accumulation, one fmaf per term, in increasing channel order, every element by one
 *   thread: no atomics, no split over the channels, run-to-run bit-identical.  A channel of weight 0 is not read at all
 *   (dead channels, NaN rows); a NaN under a non-zero weight propagates.  normalize != 0: every element is divided by the
 *   sum of the weights of the channels that contributed to it, accumulated beside it in the same order; an element without
 *   contributors (or whose contributing weights sum to 0) is 0.
 *   form: 1 = window (a workgroup owns 4 x 4 neighbouring nodes and 1024 columns, and stages per channel the contiguous span
 *   of env the tile needs in LDS, double-buffered), 2 = direct (the same loop reading env from global memory), 0 = window
 *   if the table's largest delay spread within a tile (max over tiles and channels of max d - min d over the tile's nodes)
 *   is at most 992 samples, else direct.  The choice is made on the device; both forms give the same bits.
 *   info = int32 [2], written by the call: info[0] = the form that ran (1 or 2; -1 when form = 1 was asked of a table whose
 *   spread exceeds the window, and stack is then left untouched), info[1] = that largest spread (0 with form = 2, which does
 *   not look).  info may be NULL with form = 2 only.
 * d4w_stack_best_f32: per column the largest value over the ngrid nodes and its node: peak [nt] float32, node [nt] int32.
 *   Ties go to the smallest g; a NaN never wins; a column of NaNs gives (NaN, -1).  stack = [ngrid][nt].
 * d4w_stack_arrivals_f64: Ti [ncalls][nch] float64, the form d4w_loc_solve_f64 takes.  For call c at pos[c] = (x, y, z)
 *   (pos [ncalls][3]) emitted at t0[c]: kc = floor(t0[c] fs + 0.5), m = kc + d(pos[c], ch) with the delay function above;
 *   over the samples i in [m - halfwidth, m + halfwidth] and [0, ns) the largest env[ch][i], the earliest of equals, NaNs
 *   skipped.  Ti[c][ch] = i / fs (a true division), or NaN when the window is empty, weights[ch] = 0, t0[c] is not finite, or
 *   the maximum is below the threshold: thresholds[ch] (float64 [nch]) if given, else the scalar `threshold`.
 *   One wave per (call, channel).
 * Errors: D4W_EINVAL for a NULL required pointer, nch, ns, nx, ny or ncalls < 1, pitch < ns, fs or c0 not finite or <= 0,
 *   k0 >= k1, k0 < -2^30, k1 > 2^30 or k1 - k0 > 2^31 - 1, halfwidth < 0, a form outside 0 .. 2, info = NULL with form 0 or 1,
 *   more than 65535 tiles of 4 x 4 nodes.
 * ------------------------------------------------------------------------------------------ */
int d4w_stack_delays_i32(const double* cable_pos, int nch, double c0, double fs, const double* xs, int nx, const double* ys, int ny,
                         double z, int32_t* delays, void* stream);
int d4w_stack_grid_f32(const float* env, int64_t pitch, int nch, int ns, const int32_t* delays, const float* weights, int nx, int ny,
                       int k0, int k1, int normalize, int form, float* stack, int32_t* info, void* stream);
int d4w_stack_best_f32(const float* stack, int ngrid, int nt, float* peak, int32_t* node, void* stream);
int d4w_stack_arrivals_f64(const float* env, int64_t pitch, int nch, int ns, double fs, const double* cable_pos, double c0,
                           const double* pos, const double* t0, int ncalls, int halfwidth, double threshold,
                           const double* thresholds, const float* weights, double* Ti, void* stream);

/* ------------------------------------------------------------------------------------------
 * Delay-and-sum beam of the strain toward located calls (das4whales_amd/csrc/beam.hip; the reference has
 * none of this): the waveform of a call with the array's gain.  Every pointer is DEVICE memory unless it returns a limit.
 *
 *   tau[c][ch] = |cable_pos[ch] - pos[c]| * (1 / c0) * fs      the function of csrc/moveout.h the stack's delay rounds, float64,
 *     1 / c0 formed once on the host, no contraction; pos [ncalls][3].
 *   r = (int) floor(tau + 0.5), capped at 2^30 (a NaN lands on the cap): d4w_stack_delays_i32's value at an arbitrary position.
 *   k = (int) floor(tau), f = (float)(tau - k) in [0, 1); a fraction that rounds to 1.0f is carried into k; at the cap f = 0.
 *   beam[c][j] = sum over ch, in increasing ch, of weights[ch] * v(ch, start[c] + j + delay[c][ch]),     0 <= j < length
 *     order 0: delay = r, v = x[ch][n + r]                                  one fmaf(w, x, acc) per term, as d4w_stack_grid_f32
 *     order 1: q = n + k, v = (1 - f) x[q] + f x[q + 1]
 *     order 3: four-point Lagrange on x[q - 1 .. q + 2]: l(-1) = -f (f - 1) (f - 2) / 6, l(0) = (f + 1) (f - 1) (f - 2) / 2,
 *              l(1) = -(f + 1) f (f - 2) / 2, l(2) = (f + 1) f (f - 1) / 6
 *     over the channels with weights[ch] != 0 (a channel of weight 0 is not read at all) whose taps ALL lie inside the record
 *     of ns + ns_next samples: sample ns + i of row ch is xnext[ch][i].  Everything else adds nothing.
 *   x = [nch][pitch] float32, pitch in ELEMENTS (pitch >= ns: a column-sliced view is read in place); xnext = [nch][pitch_next]
 *     or NULL (then ns_next = 0); weights [nch] float32 or NULL for ones; start [ncalls] int64, any sign.
 *   The coefficients are formed in float32 and multiplied by the weight once per (call, channel); a term of order 1 or 3 is
 *   the fmaf chain of its taps from the first product, added to the sum.  float32 sums by one thread per element and segment
 *   of 128 consecutive channels, each segment from 0 in increasing channel order, the segment partials added in increasing
 *   segment order, no atomics; with normalize the weight sums of the contributing channels take the same path and divide the
 *   element (an element without contributors is 0).  The segment is a constant of the library: a beam is run-to-run
 *   bit-identical, does not depend on the other calls of the batch, keeps its bits under a power-of-two scaling of x, and with
 *   nch <= 128, order 0 and no normalize equals d4w_stack_grid_f32's column at that node bit for bit.
 *
 * d4w_beam_limits: the largest ncalls (65535) and length (2^30) of a call, and the segment (128).
 * d4w_beam_tile: the consecutive samples one workgroup owns (what the tests size their shapes by).
 * d4w_beam_delays: k, f [ncalls][nch] (both or neither) and / or r [ncalls][nch].
 * d4w_beam_ws_bytes: the bytes of workspace d4w_beamform_f32 needs for that shape (0 with nch <= 128: ws may then be NULL).
 * d4w_beamform_f32: beam [ncalls][length] float32.  k_or_r = r with order 0 (f is not read), k otherwise.
 * Errors: D4W_EINVAL for a NULL required pointer, nch, ns, ncalls or length < 1, ncalls or length beyond the limits, more
 *   than 65535 segments of channels,
 *   pitch < ns, xnext with ns_next < 1 or pitch_next < ns_next, ns_next != 0 without xnext, fs or c0 not finite or <= 0,
 *   an order other than 0, 1, 3, order 1 or 3 without f, k without f or f without k, neither (k, f) nor r, ws = NULL where
 *   d4w_beam_ws_bytes is not 0.
 * ------------------------------------------------------------------------------------------ */
int d4w_beam_limits(int* max_calls, int* max_length, int* segment);
int d4w_beam_tile(int* samples);
int d4w_beam_delays(const double* cable_pos, int nch, double c0, double fs, const double* pos, int ncalls, int32_t* k /* or NULL */,
                    float* f /* or NULL */, int32_t* r /* or NULL */, void* stream);
int d4w_beam_ws_bytes(int nch, int ncalls, int length, size_t* bytes);
int d4w_beamform_f32(const float* x, int64_t pitch, int nch, int ns, const float* xnext /* or NULL */, int64_t pitch_next, int ns_next,
                     const int32_t* k_or_r, const float* f /* NULL for order 0 */, const float* weights /* or NULL */,
                     const int64_t* start, int ncalls, int length, int order, int normalize, float* beam, void* ws, void* stream);

/* ------------------------------------------------------------------------------------------
 * Arrival times refined against the beam (das4whales_amd/csrc/align.hip; the reference has none of this):
 * every channel correlated with the call's own waveform over 2 max_lag + 1 lags around the predicted moveout.  Every pointer
 * is DEVICE memory unless it returns a limit.
 *
 *   x, xnext, weights, start as for the beam above; tmpl [ncalls][length] float32, one template per call (the beam: its sample
 *     0 is emission sample start[c]); r [ncalls][nch] int32 = d4w_beam_delays' rounded table.
 *   n0 = start[c] + r[c][ch] in int64, start clamped to +-2^62.  For every lag m in [-max_lag, max_lag]:
 *     valid iff the samples n0 + m .. n0 + m + length - 1 all lie inside the record of ns + ns_next samples;
 *     dot[m] = sum_j tmpl[c][j] x[ch][n0 + m + j],  en[m] = sum_j x[ch][n0 + m + j]^2,  tn[c] = sum_j tmpl[c][j]^2;
 *     rho[m] = dot / sqrtf(tn en) in float32; 0 where the lag is valid but tn or en is 0; NaN where the lag is not valid (a
 *     NaN among the samples or in the template makes its entries NaN as well).
 *   The sums are float32 multiply-adds in an order that depends on length alone: dot and en one chain each over increasing j
 *   from 0; tn 64 interleaved chains (chain i over j = i, i + 64, ...) added pairwise at distances 32, 16, 8, 4, 2, 1.  rho is
 *   run-to-run bit-identical, does not depend on the other calls of the batch, and keeps its bits under a power-of-two
 *   scaling of x or of tmpl.
 *   m* = the lag of the largest non-NaN rho, the smallest m of equal values; coef = rho[m*].
 *   delta, in float64 from the float32 a = rho[m* - 1], b = rho[m*], c = rho[m* + 1]: 0.5 (a - c) / den clipped to [-0.5, 0.5]
 *     where subsample != 0, both neighbours lie within the lags and are not NaN, and den = (a - 2.0 b) + c < 0; otherwise 0.
 *   Ti[c][ch] = ((double)(n0 + m*) + delta) / fs, a true division, no contraction: the form d4w_loc_solve_f64 takes.  NaN
 *     where weights[ch] = 0, where no lag is valid or every rho is NaN, or where coef < min_coef.
 *   A channel of weight 0 is not read at all: its Ti, coef and rho row are NaN and its lag is 0.
 *
 * d4w_align_limits: the largest ncalls (65535), template length (4096) and max_lag (255) of a call, and the channels one
 *   workgroup takes (4; what the tests size their shapes by).
 * d4w_align_f32: Ti [ncalls][nch] float64 and coef [ncalls][nch] float32; lag [ncalls][nch] int32 = m* (0 where there is no
 *   lag to report: weight 0, no valid lag, every rho NaN) and rho [ncalls][nch][2 max_lag + 1] float32, each or NULL.  The
 *   pick reads the float32 rho exactly as stored in the table.  One wave per four channels of a call, no atomics.
 * Errors: D4W_EINVAL for a NULL required pointer, nch, ns or ncalls < 1, ncalls, length or max_lag beyond the limits,
 *   length < 1, max_lag < 0, pitch < ns, xnext with ns_next < 1 or pitch_next < ns_next, ns_next != 0 without xnext, fs not
 *   finite or <= 0, min_coef not finite.
 * ------------------------------------------------------------------------------------------ */
int d4w_align_limits(int* max_calls, int* max_length, int* max_lag, int* channels);
int d4w_align_f32(const float* x, int64_t pitch, int nch, int ns, const float* xnext /* or NULL */, int64_t pitch_next, int ns_next,
                  const float* tmpl, int length, const int32_t* r, const int64_t* start, int ncalls, int max_lag,
                  const float* weights /* or NULL */, double fs, double min_coef, int subsample, double* Ti, float* coef,
                  int32_t* lag /* or NULL */, float* rho /* or NULL */, void* stream);

/* ------------------------------------------------------------------------------------------
 * Robust weighted relocation (das4whales_amd/csrc/robust.hip): d4w_loc_solve_f64's damped Gauss-Newton with per-channel
 * weights and an iteratively reweighted robust loss, the second solve after d4w_align_f32 (the reference has none).
 * float64; every pointer is DEVICE memory; cable_pos, Ti, first_guess, history, n_out, gtg as for d4w_loc_solve_f64.
 *
 *   weights: NULL (ones), [nch] (weights_per_call = 0) or [ncalls][nch] (weights_per_call != 0).  Channel ch of call c is
 *     USED iff Ti[c][ch] is not NaN and its weight is > 0: a NaN, zero or negative weight means "not used".  The Ti and the
 *     cable row of an unused channel may hold anything and change no bit of any result.
 *   loss: 0 = l2, 1 = Huber, 2 = Tukey's bisquare; tuning > 0 (1.345 and 4.685 are the usual values).
 *   Iteration j = 0 .. nbiter - 1 at the iterate n, rows g and distance R as d4w_loc_solve_f64: r = Ti - (n3 + R / c0);
 *     q = 1 when loss = 0 or j < warmup; otherwise s = scale if scale > 0, else 1.4826 x the exact median of |r| over the
 *     used channels (an even count: (a + b) * 0.5 of the two middle order statistics); if s is not > 0 every q = 1; else with
 *     u = |r| / (tuning s):  Huber q = 1 for u <= 1, else 1 / u;  bisquare q = (1 - u^2)^2 for u < 1, else 0.
 *     w = weight q;  A = sum w g g^T + 1e-5 I;  b = sum w g r;  dn = A^-1 b (Cholesky);  n += 0.7 dn for j < 4, dn after.
 *   Final pass at n_out, with q as an iteration j >= warmup forms it: gtg [ncalls][p][p] = sum w g g^T without the 1e-5,
 *     ssr [ncalls] = sum w r^2, wsum [ncalls] = sum w, nused [ncalls] int32 = used channels, scale_out [ncalls] = s (NaN
 *     where no q was formed: loss = 0, or no used channel), robust_weights and residuals [ncalls][nch] = q and r per channel
 *     (NaN on unused channels).  wsum, scale_out, robust_weights and residuals each or NULL.
 *   A call without a used channel gives NaN rows in history and n_out, zeros in gtg, ssr, wsum and nused.
 *   Every sum has a fixed order and the median is integer work: run-to-run bit-identical, independent of the other calls.
 *   With loss = 0 and weights = NULL, history, n_out, gtg, ssr and nused equal d4w_loc_solve_f64's bit for bit.
 *
 * d4w_loc_robust_limits: resident_channels = the largest nch whose |r| stay in LDS for the median (above it they go through
 *   the workspace), digit_bits = the bits one pass of the radix select resolves.
 * d4w_loc_robust_ws_bytes: bytes of DEVICE scratch d4w_loc_robust_f64 needs for (nch, ncalls): 0 up to resident_channels.
 *   ws may be NULL where that is 0, and with loss = 0 or a given scale (no median is taken).
 * Errors: D4W_EINVAL for a NULL required pointer, nch < 1, ncalls < 0, c0 or tuning not positive and finite, nbiter outside
 *   0 .. 100000, nbiter > 0 without history, warmup < 0, loss outside 0 .. 2, scale neither 0 nor positive and finite,
 *   weights_per_call without weights, a missing workspace.
 * ------------------------------------------------------------------------------------------ */
int d4w_loc_robust_limits(int* resident_channels, int* digit_bits);
int d4w_loc_robust_ws_bytes(int nch, int ncalls, size_t* bytes);
int d4w_loc_robust_f64(const double* cable_pos, int nch, const double* Ti, int ncalls, const double* weights /* or NULL */,
                       int weights_per_call, double c0, int nbiter, int warmup, int fix_z, int loss, double tuning,
                       double scale /* 0: estimate */, const double* first_guess /* or NULL */, double* history, double* n_out,
                       double* gtg, double* ssr, double* wsum /* or NULL */, int* nused, double* scale_out /* or NULL */,
                       double* robust_weights /* or NULL */, double* residuals /* or NULL */, void* ws, void* stream);

/* ------------------------------------------------------------------------------------------
 * Received level of located calls per channel (das4whales_amd/csrc/levels.hip; the reference has none of
 * this): the mean square of the strain in a window that follows the call's moveout, the mean square in a noise window just
 * before it, and the largest sample of the signal window.  Every pointer is DEVICE memory unless it returns a limit.
 *
 *   x, pitch, nch, ns, xnext, pitch_next, ns_next, r, start, weights: as for d4w_align_f32 (r [ncalls][nch] int32 rounded
 *     delays, start [ncalls] int64 clamped to +-2^62; the record is ns + ns_next samples long).
 *   n0 = start[c] + r[c][ch];  signal window [n0, n0 + length);  noise window [n0 - gap - noise_length, n0 - gap).
 *   A window is valid iff it lies wholly inside the record; noise_length = 0 means no noise window.
 *     signal[c][ch] = (sum of x^2 over the signal window) / (float)length
 *     noise[c][ch]  = (sum of x^2 over the noise window) / (float)noise_length
 *     peak[c][ch]   = max |x| over the signal window (exact)
 *   float32; the sums are 64 interleaved chains (chain i takes the terms i, i + 64, ... in increasing order, one fmaf each
 *   from 0) added pairwise at distances 32, 16, 8, 4, 2, 1: an order that depends on the window length alone.
 *   An invalid window gives NaN; a NaN sample makes its window's mean square NaN; peak is NaN wherever signal is.  A channel
 *   of weight 0 is not read at all and its three outputs are NaN; a non-zero weight scales nothing.
 *
 * d4w_level_limits: the largest ncalls (65535), the largest length and noise_length + gap (2^30), and the channels one
 *   workgroup takes (4; what the tests size their shapes by).
 * d4w_level_f32: signal, noise, peak [ncalls][nch] float32; noise may be NULL iff noise_length = 0 (given, it is all NaN
 *   then).  ncalls = 0 launches nothing.  One wave per four channels of a call, no LDS, no atomics, no workspace.
 * Errors: D4W_EINVAL for a NULL required pointer (with ncalls > 0), nch or ns < 1, ncalls < 0 or beyond the limit,
 *   length < 1, noise_length < 0, gap < 0, length or noise_length + gap beyond the limit, pitch < ns, xnext with
 *   ns_next < 1 or pitch_next < ns_next, ns_next != 0 without xnext, noise = NULL with noise_length > 0.
 * ------------------------------------------------------------------------------------------ */
int d4w_level_limits(int* max_calls, int* max_length, int* channels);
int d4w_level_f32(const float* x, int64_t pitch, int nch, int ns, const float* xnext /* or NULL */, int64_t pitch_next, int ns_next,
                  const int32_t* r, const int64_t* start, int ncalls, int length, int gap, int noise_length,
                  const float* weights /* or NULL */, float* signal, float* noise /* or NULL iff noise_length == 0 */, float* peak,
                  void* stream);

/* ------------------------------------------------------------------------------------------
 * The transpose of the beam: the waveform of a located call projected back onto every channel along its moveout, fitted and
 * subtracted (das4whales_amd/csrc/project.hip; the reference has none of this).  Every pointer is DEVICE
 * memory unless it returns a limit.
 *
 *   x, pitch, nch, ns, xnext, pitch_next, ns_next, k_or_r, f, start, order: as for d4w_beamform_f32 (the tables of
 *     d4w_beam_delays: r for order 0, (k, f) for orders 1 and 3; f may be NULL for order 0; start clamped to +-2^62).
 *   beam [ncalls][length] float32: the waveform of every call, e.g. d4w_beamform_f32's normalized output.
 *   q0 = start[c] + k_or_r[c][ch];  l_m = the unweighted float32 interpolation coefficients of f[c][ch] (d4w_beamform_f32's
 *     with weight 1), m = kLo .. kHi = 0 .. 0 / 0 .. 1 / -1 .. 2 for order 0 / 1 / 3.
 *   image of the beam on the channel, the exact transpose of the beam's taps:
 *     g[c][ch](n) = sum_m l_m beam[c][n - q0 - m], beam = 0 outside 0 <= j < length; float32, t = l_lo b, then
 *     t = fmaf(l_m, b, t) in increasing m.  Support n in [q0 + kLo, q0 + length - 1 + kHi], W = length + order samples.
 *   The window is valid iff the support lies wholly inside the record of ns + ns_next samples.
 *
 * d4w_project_limits: the largest ncalls (65535), the largest length (2^30), and the channels one workgroup of the fit
 *   takes (4; what the tests size their shapes by).
 * d4w_project_f32: amp, coef [ncalls][nch] float32.  Over the support num = sum x g, den = sum g g, xx = sum x x, each a
 *   float32 sum in d4w_level_f32's order (term i of the support to chain i mod 64, one fmaf per term from 0, the chains added
 *   pairwise at distances 32 .. 1): a function of W alone.  amp = num / den (0 where den = 0), coef = num / sqrtf(den xx) (0
 *   where den or xx is 0).  An invalid window gives NaN in both and is not read; a NaN sample in the window gives NaN in both;
 *   a channel of weight 0 is not read at all and gives NaN; a non-zero weight scales nothing.  Every fit is against x as
 *   given, independent of the other calls.  ncalls = 0 launches nothing.  One wave per four channels of a call, the beam
 *   through 4 KB of LDS, no atomics, no workspace.
 * d4w_project_subtract_f32: y = x, then for c = 0, 1, ... in increasing order, where amp[c][ch] is finite and non-zero, the
 *   window is valid and n lies in its support, y[ch][n] = fmaf(-amp[c][ch], g[c][ch](n), y[ch][n]); sample ns + i of the
 *   record goes to ynext[ch][i].  ynext is given iff xnext is.  A gather: a thread owns its samples and walks the calls; no
 *   atomics, run-to-run bit-identical, independent of the launch geometry.
 *   Out of place (y != x; y, ynext must not overlap x, xnext): every sample of y and ynext is written, a copy where no call
 *   reaches (also with ncalls = 0).  In place (y = x, pitch_y = pitch; ynext = xnext, pitch_ynext = pitch_next): only the
 *   samples inside a subtracted support are read and stored; ncalls = 0 launches nothing.
 * Errors: D4W_EINVAL for a NULL required pointer (with ncalls > 0; x and y always), nch or ns < 1, ncalls < 0 or beyond the
 *   limit, length < 1 or beyond the limit, an order other than 0, 1, 3, f = NULL with order 1 or 3, a pitch below its row,
 *   xnext with ns_next < 1, ns_next != 0 without xnext, ynext without xnext or the reverse, y = x with another pitch or with
 *   ynext != xnext, ynext = xnext without y = x, more than 2^31 - 1 (channel, tile of 2048 samples) pairs.
 * ------------------------------------------------------------------------------------------ */
int d4w_project_limits(int* max_calls, int* max_length, int* channels);
int d4w_project_f32(const float* x, int64_t pitch, int nch, int ns, const float* xnext /* or NULL */, int64_t pitch_next, int ns_next,
                    const int32_t* k_or_r, const float* f /* or NULL for order 0 */, const float* beam, int length, const int64_t* start,
                    int ncalls, int order, const float* weights /* or NULL */, float* amp, float* coef, void* stream);
int d4w_project_subtract_f32(const float* x, int64_t pitch, int nch, int ns, const float* xnext /* or NULL */, int64_t pitch_next, int ns_next,
                             const int32_t* k_or_r, const float* f /* or NULL for order 0 */, const float* beam, int length,
                             const int64_t* start, const float* amp, int ncalls, int order, float* y, int64_t pitch_y,
                             float* ynext /* or NULL iff xnext is */, int64_t pitch_ynext, void* stream);

/* ------------------------------------------------------------------------------------------
 * Coherence of located calls along their moveout: windowed semblance of the beam and phase coherence of the analytic signal
 * (das4whales_amd/csrc/coherence.hip; the reference has none of this).  Every pointer is DEVICE memory unless
 * it returns a limit.
 *
 *   x, pitch, nch, ns, xnext, pitch_next, ns_next, k_or_r, f, weights, start, order: as for d4w_beamform_f32, with
 *     weights[ch] >= 0 and finite.  ximag [nch][pitch_imag] or NULL: the imaginary part of the analytic signal of x (its
 *     Hilbert transform), the same nch and ns; ximag_next [nch][pitch_imag_next]: that of xnext, given iff both are.
 *   For call c, channel ch of weight w = weights[ch] and beam sample j, n = start[c] + j:
 *     v(ch, j) = the record at n + delay[c][ch], interpolated exactly as d4w_beamform_f32 does for order 0, 1, 3;
 *     h(ch, j) = the same interpolation of the imaginary block.
 *     A term exists iff all of its taps lie inside the record [0, ns + ns_next); a channel of weight 0 is not read.
 *   Over the contributing channels, in increasing order:
 *     b[c][j] = sum w v          e[c][j] = sum w v^2          W[c][j] = sum w
 *     pr = sum w v / a           pi = sum w h / a             a = sqrt(v^2 + h^2); a term with a = 0 adds nothing to pr, pi
 *                                                             (its w stays in W)
 *     semblance[c][j] = sum_tau b^2 / sum_tau (W e),  tau over [j - H, j + H] clipped to [0, length);  0 where the denominator is 0
 *     phase[c][j]     = sqrt(pr^2 + pi^2) / W;  0 where W is 0
 *   Both lie in [0, 1] (Cauchy-Schwarz per tau with w >= 0) up to float32 rounding.
 *   float32 throughout: channel sums in increasing channel order in fixed segments of 128 channels, the segment partials
 *   added in increasing order; window sums add their 2H + 1 terms in increasing tau; no running sums, no atomics: run-to-run
 *   bit-identical and independent of the other calls of the batch.  The term w v is the beam's, so beam is bit for bit what
 *   d4w_beamform_f32(normalize = 0) writes for the same arguments; e adds fmaf(t / w, t, e) with t = w v.  semblance keeps
 *   its bits under a power-of-two scaling of x, absent underflow.  a = 0 means: the float32 v^2 + h^2 (of the weighted
 *   terms) is below 2^-126.  Non-finite samples under a non-zero weight leave the elements they touch unspecified.
 *
 * d4w_coherence_limits: the largest ncalls (65535), length (2^30) and half window H (256), and the segment (128).
 * d4w_coherence_ws_bytes: the bytes of workspace for that shape, phase = whether an imaginary block is given (never 0).
 * d4w_coherence_f32: beam, semblance [ncalls][length]; phase [ncalls][length], given iff ximag is; wsum [ncalls][length]
 *   (W) or NULL.  A NULL output is not written.
 * d4w_coherence_peak_f32: per call the largest semblance over the columns [lo, hi) and the smallest column that attains it
 *   (peak NaN and index -1 where the range holds nothing but NaN).
 * Errors: D4W_EINVAL for a NULL required pointer (ws included), the shape and record errors of d4w_beamform_f32, an order
 *   other than 0, 1, 3, order 1 or 3 without f, H outside 0 .. the limit, ximag without phase or the reverse, a pitch of an
 *   imaginary block below its row, ximag_next without ximag, ximag_next given without xnext or missing with it, a weight that
 *   is negative or not finite (the weights are copied to the host for this: the call waits for the stream when weights
 *   are given), a peak range not inside [0, length).  Every error is reported before any launch.
 * ------------------------------------------------------------------------------------------ */
int d4w_coherence_limits(int* max_calls, int* max_length, int* max_half_window, int* segment);
int d4w_coherence_ws_bytes(int nch, int ncalls, int length, int phase, size_t* bytes);
int d4w_coherence_f32(const float* x, int64_t pitch, int nch, int ns, const float* xnext /* or NULL */, int64_t pitch_next, int ns_next,
                      const float* ximag /* or NULL */, int64_t pitch_imag, const float* ximag_next /* or NULL */,
                      int64_t pitch_imag_next, const int32_t* k_or_r, const float* f /* NULL for order 0 */,
                      const float* weights /* or NULL */, const int64_t* start, int ncalls, int length, int order, int half_window,
                      float* beam, float* semblance, float* phase /* or NULL iff ximag is */, float* wsum /* or NULL */, void* ws,
                      void* stream);
int d4w_coherence_peak_f32(const float* semblance, int ncalls, int length, int lo, int hi, float* peak, int32_t* index, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* D4W_H */
