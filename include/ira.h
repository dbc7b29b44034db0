/*
 * ira.h -- C-ABI of libira.so: batched impulse-response analysis kernels for AMD MI355X (gfx950).
 *
 * The reference project (kianmcevoy/audio_analysis) is pure Python and has no FFI for this path
 * (SURVEY.md section 8b); the boundary it exposes is its per-module Python API.  Each entry point
 * below therefore cites the reference Python function whose numeric body it replaces, and
 * INTEGRATION.md shows the ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *  - extern "C", plain pointers and sizes, no exceptions, no torch types.
 *  - Every pointer named *_dev is DEVICE memory owned by the caller (the Python host allocates
 *    torch-ROCm tensors and passes data_ptr()).  The library allocates nothing the caller sees and
 *    keeps no state: all tables (windows, twiddles) are caller-provided device buffers.
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream).  Calls only enqueue work;
 *    they never synchronise.  Re-entrant per stream.
 *  - Ragged batches: a flat float32 sample buffer plus per-segment int64 offset/length arrays.
 *  - Return value: 0 = ok; negative = argument error (IRA_E_*); <= -1000 = -(1000 + hipError_t).
 */
#ifndef IRA_H_
#define IRA_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IRA_OK 0
#define IRA_E_NULL (-1)       /* a required pointer was NULL */
#define IRA_E_SIZE (-2)       /* a size/shape argument is out of the supported range */
#define IRA_E_UNSUPPORTED (-3)
#define IRA_E_IO (-4)         /* a file could not be opened or read (host-side ingest entry points only) */
#define IRA_E_FORMAT (-5)     /* a file is not RIFF/WAVE (host-side ingest entry points only) */
#define IRA_E_HIP_BASE (-1000)

#define IRA_ABI_VERSION 15  /* bumped whenever an exported signature or a scratch-size constant changes */

int32_t ira_abi_version(void);
const char* ira_error_string(int32_t code);

/* ---- a2: peak pick ---------------------------------------------------------------------------
 * peak_dev[s] = argmax_n |x[off[s]+n]|, n < len[s]; the FIRST maximum wins (bit-exact integer); a NaN beats every number
 * and the first NaN wins whatever its payload (peak_abs_dev[s] is then NaN).
 * Replaces np.argmax(np.abs(x)) at reference analyse/decay.py:136, spectrogram.py:181,
 * waterfall.py:359, modalcloud.py:299, frequency_response.py:186, filterplot.py:125,
 * zplane.py:197, rt60bands.py:335.  Also returns the peak magnitude (zplane.py:211).
 * max_len = longest segment (sizes the grid; every sample of every segment is visited; < 2^32); nseg <= 65535. */
int32_t ira_peak_index(const float* x_dev, const int64_t* off_dev, const int64_t* len_dev,
                       int32_t nseg, int64_t max_len, int64_t* peak_dev, float* peak_abs_dev, void* stream);

/* ---- a3: Schroeder energy-decay curve ----------------------------------------------------------
 * For each segment: e = x^2 (f64) -> reverse cumulative sum -> max(.,eps) -> /edc[0] -> 10 log10
 * -> max(.,floor_db) -> float32, written to edc_db_dev at the same offsets as the input segment
 * (edc_off_dev).  Replaces compute_schroeder_edc_db, reference analyse/decay.py:115-170
 * edc_db64_dev (optional, may be NULL): the same curve as float64 BEFORE the floor, for the optional
 * host-side dB smoothing of decay.py:161-164.  edc_db_dev may be NULL if only that is wanted.
 * max_len = longest segment (sizes the grid; up to 2047 tiles of 4096 samples = 8.38 M samples).
 * scratch_dev: nseg * IRA_EDC_SCRATCH_DOUBLES doubles. */
#define IRA_EDC_SCRATCH_DOUBLES 4096
int32_t ira_edc_db(const float* x_dev, const int64_t* off_dev, const int64_t* len_dev, int32_t nseg,
                   int64_t max_len, double eps, double floor_db, float* edc_db_dev, double* edc_db64_dev,
                   const int64_t* edc_off_dev, double* scratch_dev, void* stream);

/* ---- a4/a5/a16: threshold crossings + straight-line decay fits on a float32 dB curve -------------
 * For each curve c (ncurves of them) and each of nranges (hi_db, lo_db_effective) pairs:
 *   first index with y <= target (float32 compare), linear interpolation of the crossing time in
 *   f64, mask t>=t_start & t<=t_end in float32, >= min_points, least-squares line, slope<0, r^2,
 *   rt60 = -60/slope.
 * Replaces _interpolated_crossing_time_seconds + fit_decay_slope_over_db_range, reference
 * analyse/decay.py:173-260, and the per-bin copy analyse/modalcloud.py:215-281.
 * Time axis: t[i] = float32(i) * t_mul / t_div evaluated in float32 exactly like the reference
 * (decay.py:169: t_mul = 1, t_div = sr; spectrogram.py:158: t_mul = hop, t_div = sr).
 * If t_axis_dev != NULL it is an explicit float32 time axis (>= max_len values, shared by all curves)
 * used instead of the analytic one (the public fit_decay_slope_over_db_range takes any time array).
 * If rel_to_peak != 0 the curve is first shifted by its own maximum in float32
 * (modalcloud.py:356-361) and curves that are not finite or whose peak - floor_db <
 * min_peak_above_floor are flagged invalid (status bit 2).
 * ranges_hi_lo (2*nranges doubles) and cross_targets are HOST arrays; nranges <= 4, ncross <= 4;
 * max_len (longest curve) only picks the workgroup size.
 * cross_targets (ncross values) -> cross_out_dev[c*ncross + j] crossing time or NaN
 * (used for the 0 / -10 dB early-decay time, decay.py:280-286).
 * fit_out_dev: ncurves*nranges records of IRA_FIT_DOUBLES doubles:
 *   [0] valid (1/0) [1] start_t [2] end_t [3] slope [4] intercept [5] r2 [6] rt60 [7] npts */
#define IRA_FIT_DOUBLES 8
int32_t ira_curve_fits(const float* y_dev, const int64_t* off_dev, const int64_t* len_dev,
                       int32_t ncurves, int32_t max_len, float t_mul, float t_div,
                       const float* t_axis_dev, const double* ranges_hi_lo,
                       int32_t nranges, int32_t min_points, const double* cross_targets,
                       int32_t ncross, int32_t rel_to_peak, double floor_db,
                       double min_peak_above_floor, double* fit_out_dev, double* cross_out_dev,
                       void* stream);

/* Optional dB smoothing of the EDC (reference analyse/decay.py:159-166, default off): out[s][i] = float32(max(floor_db,
 * numpy.convolve(edc_db64[s], ones(window)/window, mode="same")[i])) on the unfloored float64 curve ira_edc_db writes
 * (edc_db64_dev); in and out share the offsets off_dev.  IRA_E_UNSUPPORTED when window > max_len.  The function sees the
 * lengths on the device only: a segment of a ragged batch that is shorter than the window (where numpy's "same" returns
 * `window` values instead of len) is NOT refused, its sums are clipped to the segment; the caller refuses such a request
 * (analyse/decay.py and analyse/rt60bands.py raise ValueError when any analysed length is shorter than the window). */
int32_t ira_edc_box_smooth(const double* edc_db64_dev, const int64_t* off_dev, const int64_t* len_dev, int32_t nseg,
                           int64_t max_len, int32_t window, double floor_db, float* out_dev, void* stream);

/* ---- a3-a6 fused: Schroeder EDC -> crossings -> decay-line fits, straight from the samples --------------------------
 * The same results as ira_edc_db followed by ira_curve_fits (analytic time axis t[i] = float32(i)*t_mul/t_div, no
 * rel_to_peak), without reading an EDC array: per segment the chunk sums locate each target level, only the
 * chunks around the crossings and between them are re-scanned (identical float32 dB values, same code as the emit
 * pass), and the regression is one sweep of shifted float64 moments.  Replaces, for one segment, the call chain
 * compute_schroeder_edc_db -> _interpolated_crossing_time_seconds -> fit_decay_slope_over_db_range of
 * analyse_decay_for_channel (reference analyse/decay.py:268-329) and of every band of
 * _compute_band_metrics_from_samples (analyse/rt60bands.py:272-321), whose EDC curve is never a result.
 * edc_db_dev (optional, may be NULL): also write the float32 dB curve at edc_off_dev[s] (the decay block returns it).
 * fit_out_dev / cross_out_dev: records exactly as ira_curve_fits writes them.  ranges_hi_lo / cross_targets: HOST arrays.
 * scratch_dev: nseg * IRA_EDC_SCRATCH_DOUBLES doubles.  max_len as for ira_edc_db.
 * tile_part_dev (optional, may be NULL; round 5): partial tile energies a producer of the segments left behind
 * (ira_band_irfft_smooth, tile_part_dev): segment s with part_off_dev[s] >= 0 takes the energy of its tile j (4096 samples,
 * counted from the END of the segment) as the sum over w < part_wgs_dev[s] of tile_part_dev[part_off_dev[s] +
 * w * part_tiles_dev[s] + j] (part_tiles_dev[s] = tiles of the producer's whole signal), for every tile but the one that holds its first sample (that one is scanned, so that edc[0] stays
 * the value the curve has at index 0) -- instead of reading its samples once more (rt60bands.py:272-321 through
 * decay.py:115-170: a band's signal is written by the inverse transform a moment earlier).  CONTRACT: such a segment ends
 * where the producer's signal ends (a band signal from its start index on).  part_off_dev[s] < 0: the samples are read. */
int32_t ira_edc_fits(const float* x_dev, const int64_t* off_dev, const int64_t* len_dev, int32_t nseg,
                     int64_t max_len, double eps, double floor_db, float t_mul, float t_div,
                     const double* ranges_hi_lo, int32_t nranges, int32_t min_points,
                     const double* cross_targets, int32_t ncross, double* fit_out_dev, double* cross_out_dev,
                     float* edc_db_dev, const int64_t* edc_off_dev, double* scratch_dev, const double* tile_part_dev,
                     const int64_t* part_off_dev, const int32_t* part_wgs_dev, const int32_t* part_tiles_dev,
                     void* stream);

/* ---- a11: STFT magnitude in dB -------------------------------------------------------------------
 * Valid framing (no padding), frame f of segment s starts at off[s] + f*hop, nframes[s] frames.
 * out[s] is a C-contiguous (n_fft/2+1, nframes[s]) float32 matrix at out_dev + out_off[s]:
 *   20*log10(max(|rfft(frame*window)|, 10^(floor_db/20))).
 * Replaces _compute_stft_magnitude_db, reference analyse/spectrogram.py:107-160 and its copies
 * analyse/waterfall.py:188-230, analyse/modalcloud.py:121-158.
 * precision: 32 = float32 butterflies (spectrogram), 64 = float64 butterflies.
 * window_dev: n_fft values; twiddle_dev: n_fft/2 interleaved (cos, -sin) pairs of
 * exp(-2*pi*i*k/n_fft); both float (precision 32) or double (precision 64).
 * frame_sel_dev (optional): if not NULL, nframes[s] is the number of SELECTED frames and
 * frame_sel_dev[sel_off[s] + j] gives the frame index of output column j (waterfall shortcut,
 * reference analyse/waterfall.py:309). n_fft: power of two, 64..16384. */
int32_t ira_stft_mag_db(const float* x_dev, const int64_t* off_dev, const int32_t* nframes_dev,
                        int32_t nseg, int32_t max_frames, int32_t n_fft, int32_t hop,
                        const void* window_dev, const void* twiddle_dev, int32_t precision,
                        double floor_db, float* out_dev, const int64_t* out_off_dev,
                        const int32_t* frame_sel_dev, const int64_t* sel_off_dev, void* stream);

/* Same transform, FRAME-MAJOR output: out[e] is a (T_e, n_fft/2+1) matrix, i.e. the transpose of the reference's
 * (F, T) array -- every frame's bins are contiguous, which lets each wave store its frame directly (no transposing
 * tile, no partial-line writes).  For device-resident consumers and hosts that take a `.T` view.  Implemented for
 * precision 32 / n_fft 4096 and precision 64 / n_fft 8192 (the reference's spectrogram and modal-cloud defaults);
 * anything else returns IRA_E_UNSUPPORTED (use ira_stft_mag_db). */
int32_t ira_stft_mag_db_tf(const float* x_dev, const int64_t* off_dev, const int32_t* nframes_dev,
                           int32_t nseg, int32_t max_frames, int32_t n_fft, int32_t hop,
                           const void* window_dev, const void* twiddle_dev, int32_t precision,
                           double floor_db, float* out_dev, const int64_t* out_off_dev,
                           const int32_t* frame_sel_dev, const int64_t* sel_off_dev, void* stream);

/* STFT + modal-cloud log-bin aggregation in ONE kernel (ira_stft_mag_db followed by ira_logbin_aggregate, with the dB
 * matrix never written): curves_dev[e] is the (nbins, T_e) float32 matrix at curves_off_dev[e]; k_base / first / count
 * as in ira_logbin_aggregate (every row k_base + first[b] + j must be < n_fft/2 + 1).  Same arithmetic, including the
 * float32 rounding of the dB value before it is converted back to linear magnitude.  precision 64 / n_fft 8192 only
 * (IRA_E_UNSUPPORTED otherwise).  Replaces reference analyse/modalcloud.py:121-158 + :176-207 for the modal cloud. */
int32_t ira_stft_logbin(const float* x_dev, const int64_t* off_dev, const int32_t* nframes_dev, int32_t nseg,
                        int32_t max_frames, int32_t n_fft, int32_t hop, const void* window_dev,
                        const void* twiddle_dev, int32_t precision, double floor_db, int32_t k_base,
                        const int32_t* first_dev, const int32_t* count_dev, int32_t nbins, float* curves_dev,
                        const int64_t* curves_off_dev, void* stream);

/* ---- suffix energies, and the two STFT calls above certified from them ---------------------------------------------
 * ira_tail_energy: per segment s the float64 table S at tab_dev + tab_off[s], nblk[s] + 1 doubles with
 * nblk[s] = ceil((end[s] - start[s]) / IRA_TAIL_BLOCK):
 *   S[j] = sum of x[n]^2 over n in [start[s] + j IRA_TAIL_BLOCK, end[s]),  S[nblk[s]] = 0
 * (start / end: sample indices into x_dev; end is where the segment's channel ends, nothing is read at or past it).
 * Exact squares added in a fixed order: the same inputs give the same bits in every run.  A NaN or an infinity makes every
 * entry at or before its block non-finite and leaves the entries behind it alone.  max_nblk = the largest nblk[s] (sizes
 * the grid); nseg <= 65535.  Nothing in the reference computes this table: it exists for the two calls below. */
#define IRA_TAIL_BLOCK 512
int32_t ira_tail_energy(const float* x_dev, const int64_t* start_dev, const int64_t* end_dev,
                        const int64_t* tab_off_dev, int32_t nseg, int32_t max_nblk, double* tab_dev, void* stream);

/* ira_stft_logbin / ira_stft_mag_db_tf (their configurations) with the table of ira_tail_energy: THE SAME BYTES as the
 * call without it.  A frame (precision 32) or a workgroup's run of frames (precision 64) that starts in block j of its
 * segment reads only samples S[j] covers, so 4 n_fft max(window^2) S[j] <= floor^2 certifies that it is floored on every
 * row, with one load and no sample traffic; nothing is certified from a non-finite entry.
 * CONTRACT: tail_dev / tail_off_dev are the table and offsets of an ira_tail_energy call whose start[s] == off[s] for
 * every segment, and no frame of segment s reads at or past that call's end[s].  tail_dev == NULL: exactly the call
 * without the table.  With a frame selection the table is ignored.
 * consts_dev: scratch the precision-64 call fills for itself (the window's greatest square and the floored log-bin row),
 * IRA_STFT_CONSTS_DOUBLES(nbins) doubles (nbins = 0 for ira_stft_mag_db_tf_tail); required with a table there. */
#define IRA_STFT_CONSTS_DOUBLES(nbins) (1 + ((nbins) + 1) / 2)
int32_t ira_stft_logbin_tail(const float* x_dev, const int64_t* off_dev, const int32_t* nframes_dev, int32_t nseg,
                             int32_t max_frames, int32_t n_fft, int32_t hop, const void* window_dev,
                             const void* twiddle_dev, int32_t precision, double floor_db, int32_t k_base,
                             const int32_t* first_dev, const int32_t* count_dev, int32_t nbins, float* curves_dev,
                             const int64_t* curves_off_dev, const double* tail_dev, const int64_t* tail_off_dev,
                             void* consts_dev, void* stream);
int32_t ira_stft_mag_db_tf_tail(const float* x_dev, const int64_t* off_dev, const int32_t* nframes_dev,
                                int32_t nseg, int32_t max_frames, int32_t n_fft, int32_t hop,
                                const void* window_dev, const void* twiddle_dev, int32_t precision,
                                double floor_db, float* out_dev, const int64_t* out_off_dev,
                                const int32_t* frame_sel_dev, const int64_t* sel_off_dev, const double* tail_dev,
                                const int64_t* tail_off_dev, void* consts_dev, void* stream);

/* ---- a9/a17: arbitrary-length float64 DFTs (Bluestein over a four-step FFT of size M) -------------------
 * Common arguments: the convolution size m = M, a power of two (16 <= M <= 2^22) or three times one
 * (96 <= M <= 3*2^20), with M >= 2*max(L) - 1 -- or only M >= L + L/2 for ira_rfft_any elements that carry ONE real
 * signal (no x2off / interleave): their L/2+1 bins do not see the wrap-around; three caller-provided
 * complex-f64 tables for M = N1*N2 with the split ira_fft_split() reports (N2 a power of two, N1 one or 3x one):
 *   t1_dev[k] = exp(-2 pi i k/N1), k < N1;  t2_dev[k] = exp(-2 pi i k/N2), k < N2;
 *   tf_dev[k] = exp(-2 pi i k/M),  k < N2.
 * work_dev: nb * M complex f64 of scratch.  bfilt_dev: chirp-filter spectra built by ira_bluestein_filter
 * FOR THE SAME M, M complex f64 each; bidx_dev[e] selects the filter (the one built for length L[e]) of element e. */

/* The four-step split the library uses for size m (host code sizes t1/t2/tf from it); IRA_E_SIZE if m is not a
 * supported size.  No reference counterpart: numpy's pocketfft plans internally (reference
 * analyse/frequency_response.py:204). */
int32_t ira_fft_split(int32_t m, int32_t* n1, int32_t* n2);

/* bfilt_dev[j] = FFT_M of the Bluestein chirp filter for length L_dev[j], j < nfilt. */
int32_t ira_bluestein_filter(const int32_t* L_dev, int32_t nfilt, int32_t m, const void* t1_dev,
                             const void* t2_dev, const void* tf_dev, double* bfilt_dev, void* stream);

/* spec_out[e][k] = sum_n x[xoff[e]+n] * (hanning(L[e])[n] | 1) * exp(-2 pi i n k / L[e]),  k = 0..L[e]/2,
 * complex f64 at spec_out_dev + 2*spec_off_dev[e] doubles.  Replaces np.fft.rfft(x * w) of arbitrary
 * length at reference analyse/frequency_response.py:204-213, analyse/filterplot.py:145-152 and the
 * forward transform of analyse/rt60bands.py:172.
 * Two real signals of the SAME length can share one transform (z = x1 + i*x2, split by Hermitian symmetry):
 * x2off_dev (may be NULL = no pairs) gives the second signal of element e or -1; its spectrum goes to
 * spec_off2_dev[e]; zpair_dev/zpair_off_dev is scratch for the full-length complex DFT (L[e] complex f64 per
 * paired element) and max_len >= max L[e].  Cross-talk between the two signals is at the 1e-16 level of the
 * larger one.
 * Zero-padded / truncated transforms, numpy.fft.rfft(x * hanning(len(x)), n=L) (reference
 * analyse/group_delay.py:95-109): data_len_dev[e] (may be NULL = L[e]) samples are read, the rest of the L[e]
 * inputs are zero (data_len > L truncates), and the Hann window is the one of length win_len_dev[e] (NULL =
 * L[e]); data_len2_dev / win_len2_dev (NULL = same as the first) apply to the second signal of a pair.
 * interleave_dev (may be NULL): interleave[e] = 1 makes element e ONE real signal of even length 2*L[e] carried as the
 * complex sequence x[2m] + i*x[2m+1] (x2off_dev[e] must be xoff_dev[e] + 1, zpair scratch L[e] complex): half the
 * transform size; its L[e]+1 spectrum bins go to spec_off_dev[e].  Window lengths then refer to the real signal
 * (win_len = 2*L[e]).
 * keep_packed != 0 (round 4): the L[e]-point transforms Z of interleaved elements are NOT untangled -- they stay where
 * the last pass wrote them, zpair_dev + 2*zpair_off_dev[e] (the caller may point that into spec_out_dev: L[e] values fit
 * the element's L[e]+1 bins), and the consumer forms X[k] = E[k] + W^k O[k] as it reads them
 * (ira_spectrum_mag_phase, packed_dev): one read-modify-write pass over every such spectrum less.  Such a call must not
 * carry paired elements (x2off_dev[e] >= 0 only where interleave_dev[e] = 1): no split kernel is launched at all.
 * keep_packed with x2off_dev but WITHOUT interleave_dev (every second signal would be a paired one) returns
 * IRA_E_UNSUPPORTED. */
int32_t ira_rfft_any(const float* x_dev, const int64_t* xoff_dev, const int32_t* L_dev, int32_t nb,
                     int32_t use_hann, int32_t m, const void* t1_dev, const void* t2_dev,
                     const void* tf_dev, const double* bfilt_dev, const int32_t* bidx_dev,
                     double* work_dev, double* spec_out_dev, const int64_t* spec_off_dev,
                     const int64_t* x2off_dev, const int64_t* spec_off2_dev, double* zpair_dev,
                     const int64_t* zpair_off_dev, int32_t max_len, const int32_t* data_len_dev,
                     const int32_t* win_len_dev, const int32_t* data_len2_dev, const int32_t* win_len2_dev,
                     const int32_t* interleave_dev, int32_t keep_packed, void* stream);

/* Band filter bank: element e takes the half spectrum at spec_dev + 2*spec_off_dev[e] (length L[e]/2+1),
 * multiplies it by TWO real masks (band_params_dev: 2 records of IRA_BAND_DOUBLES doubles per element:
 * [0] kind 0 none/1 low-pass/2 high-pass/3 band-pass, [1] hp ramp start, [2] hp ramp end (pass edge),
 * [3] lp ramp start (pass edge), [4] lp ramp end; masks are evaluated in float32 on the float32 axis
 * float32(k*freq_val[e]) exactly as reference analyse/rt60bands.py:116-167) and inverse-transforms both
 * at once (y1 + i*y2), writing float32 signals of length L[e] at y_dev + y1_off[e] and y_dev + y2_off[e]
 * (y2_off[e] < 0: no second band).  spec_off2_dev (may be NULL) lets the SECOND band come from another
 * spectrum of the same length and bin step (e.g. the odd band of two different channels share one inverse
 * transform): band 2 of element e then filters spec_dev + 2*spec_off2_dev[e].  Replaces _apply_fft_mask, reference analyse/rt60bands.py:170-175. */
#define IRA_BAND_DOUBLES 8
int32_t ira_band_irfft(const double* spec_dev, const int64_t* spec_off_dev, const int32_t* L_dev,
                       int32_t nb, const double* band_params_dev, const double* freq_val_dev,
                       int32_t m, const void* t1_dev, const void* t2_dev, const void* tf_dev,
                       const double* bfilt_dev, const int32_t* bidx_dev, double* work_dev, float* y_dev,
                       const int64_t* y1_off_dev, const int64_t* y2_off_dev,
                       const int64_t* spec_off2_dev, void* stream);

/* ---- a17/a18: spectrum post-processing -------------------------------------------------------------------
 * mag_db[e][k] = float32(20 log10(max(|X|, 10^(floor_db/20)))), optional phase[e][k] = atan2(im, re) (f64).
 * Reference analyse/frequency_response.py:213-218, analyse/filterplot.py:152-160.
 * packed_dev (may be NULL): packed[e] != 0 says element e (even L[e]) is still the PACKED half-length transform
 * Z = DFT(x[2m] + i x[2m+1]) of L[e]/2 values (ira_rfft_any, keep_packed) at spec_off_dev[e]; its L[e]/2+1 bins are formed
 * on the fly. */
int32_t ira_spectrum_mag_phase(const double* spec_dev, const int64_t* spec_off_dev, const int32_t* L_dev,
                               int32_t nb, int32_t max_len, double floor_db, float* mag_db_dev,
                               const int64_t* mag_off_dev, double* phase_dev,
                               const int64_t* phase_off_dev, const int32_t* packed_dev, void* stream);

/* numpy.unwrap (optional) + rad2deg (optional) -> float32 (out_dev, may be NULL), and/or the unwrapped phase in
 * float64 radians (out64_dev, may be NULL; same offsets).  Reference analyse/filterplot.py:162-168 and
 * analyse/group_delay.py:113-115. */
int32_t ira_phase_unwrap(const double* phase_dev, const int64_t* phase_off_dev, const int32_t* L_dev,
                         int32_t nb, int32_t do_unwrap, int32_t to_degrees, float* out_dev,
                         const int64_t* out_off_dev, double* out64_dev, void* stream);

/* Section 8f, group delay: gd[e][k] = -numpy.gradient(phase[e], w)[k] with w[k] = 2 pi ((k * bin_step[e]) /
 * sample_rate) in rad/sample, k < nbins[e]; numpy's rule "uniform formula only if every diff(w) is bit-identical,
 * three-point non-uniform formula otherwise" is reproduced (flags_dev: nb int32 of scratch, 1 = non-uniform).
 * phase/gd share off_dev (float64 elements).  Replaces the gradient step of _compute_group_delay_from_ir,
 * reference analyse/group_delay.py:117-124.   flags_known != 0 (round 4): flags_dev already holds, per element, whether numpy.gradient takes the
 * non-uniform formula (a function of bins, bin step and sample rate alone: callers decide it once per transform length);
 * the sweep that works it out on the device is skipped. */
int32_t ira_group_delay(const double* phase_dev, const int64_t* off_dev, const int32_t* nbins_dev, int32_t nb,
                        int32_t max_bins, const double* bin_step_dev, double sample_rate_hz, int32_t* flags_dev,
                        int32_t flags_known, double* gd_dev, void* stream);

/* Statistics over bins with f_min <= float32(k*freq_val[e]) <= f_max (float32 compares): out_dev[e*8..]:
 * [0] bin count [1] argmax bin of mag_db (first max) [2] its frequency [3] sum f*10^(dB/20) [4] sum 10^(dB/20)
 * [5] first in-range frequency [6] argmin |f - probe_hz| over ALL bins (first min) [7] mag_db there.
 * Reference analyse/frequency_response.py:238-260, analyse/filterplot.py:173-191. */
int32_t ira_spectrum_stats(const float* mag_db_dev, const int64_t* mag_off_dev, const int32_t* L_dev,
                           int32_t nb, const double* freq_val_dev, double f_min_hz, double f_max_hz,
                           double probe_hz, double* out_dev, void* stream);

/* ira_spectrum_mag_phase, ira_phase_unwrap and ira_spectrum_stats in ONE pass over every spectrum (one launch; the wrapped
 * phase never goes through memory, the dB values are not read back).  Every output sits at out_off_dev[e] (elements of its
 * own type) and may be NULL, at least one of mag_db_dev / phase32_dev / phase64_dev / wrapped64_dev is not; what nobody wants
 * is not computed.  mag_db_dev: as ira_spectrum_mag_phase (floor_db, packed_dev).  phase32_dev: float32 of the (unwrapped if
 * do_unwrap) phase, in degrees if to_degrees; phase64_dev: the same in float64 radians; wrapped64_dev: the angles before the
 * unwrap.  stats_dev (needs mag_db_dev and freq_val_dev, IRA_E_NULL otherwise): the records of ira_spectrum_stats over the
 * dB values written.  For plain half spectra every output has the bytes of the three calls; a packed element's bins are
 * formed with another (shorter) chain of roundings in the twiddle than ira_spectrum_mag_phase's. */
int32_t ira_spectrum_finish(const double* spec_dev, const int64_t* spec_off_dev, const int32_t* L_dev, int32_t nb,
                            double floor_db, const int32_t* packed_dev, float* mag_db_dev, const int64_t* out_off_dev,
                            int32_t do_unwrap, int32_t to_degrees, float* phase32_dev, double* phase64_dev,
                            double* wrapped64_dev, const double* freq_val_dev, double f_min_hz, double f_max_hz,
                            double probe_hz, double* stats_dev, void* stream);

/* ---- a14: waterfall slice normalisation ----------------------------------------------------------------
 * mag[e] is the (F, S_e) STFT dB matrix of the S_e selected frames (ira_stft_mag_db with frame_sel_dev);
 * out[e] is (S_e, nsel) float32: clip(mag[k_lo+k, s] - ref, -dyn_db, 0), ref = max over the selected block
 * (slice_max = 0) or over each slice (slice_max = 1), float32 arithmetic.
 * Replaces _build_rel_db_slices, reference analyse/waterfall.py:289-341 (smoothing off). */
int32_t ira_waterfall_rel(const float* mag_dev, const int64_t* mag_off_dev, const int32_t* nslices_dev,
                          int32_t nb, int32_t k_lo, int32_t nsel, int32_t slice_max, double dyn_db,
                          float* out_dev, const int64_t* out_off_dev, void* stream);

/* ---- a15: modal-cloud log-frequency aggregation -----------------------------------------------------------
 * mag[e] is the (F, T_e) STFT dB matrix; for log bin b rows k_base+first[b] .. +count[b]-1 are averaged as
 * linear magnitude 10^(dB/20) in float64 (rows added in order), then 20 log10(max(mean, 1e-30)) -> float32;
 * count[b] == 0 gives a NaN row; a NaN among a frame's rows of a bin stays NaN (numpy.maximum), it is not clamped.
 * out[e] is (nbins, T_e).  frame_major_rows > 0: mag[e] is the FRAME-MAJOR (T_e, F)
 * matrix of ira_stft_mag_db_tf with F = frame_major_rows <= 8193 (same results, same row order).
 * Replaces _aggregate_to_log_bins, reference analyse/modalcloud.py:176-207. */
int32_t ira_logbin_aggregate(const float* mag_dev, const int64_t* mag_off_dev, const int32_t* nframes_dev,
                             int32_t nb, int32_t max_frames, int32_t k_base, const int32_t* first_dev,
                             const int32_t* count_dev, int32_t nbins, float* out_dev,
                             const int64_t* out_off_dev, int32_t frame_major_rows, void* stream);

/* Optional log-frequency smoothing of dB curves IN PLACE (reference analyse/waterfall.py:140-185 and
 * analyse/frequency_response.py:117-169; default off): curve c = the bins k_lo[c] .. k_lo[c]+nsel[c]-1 (frequencies
 * float32(k * fstep[c])) of the float32 array at mag_dev + off[c], consecutive bins stride[c] elements apart.  They are
 * interpolated (numpy.interp) onto count[c] points uniform in log2(f) between log2_lo[c] and log2_hi[c] (the host computes
 * numpy.log2 of the first / last selected frequency and the count), averaged with a `window`-point box
 * (numpy.convolve(.., "same")), interpolated back and cast to float32.  through_float32 != 0: the waterfall variant, which
 * casts the gridded curve to float32 before and after the convolution.  max_count = largest count (<= 2048, else
 * IRA_E_UNSUPPORTED). */
int32_t ira_log_smooth_db(float* mag_dev, const int64_t* off_dev, const int32_t* stride_dev, const int32_t* k_lo_dev,
                          const int32_t* nsel_dev, const double* fstep_dev, const double* log2_lo_dev,
                          const double* log2_hi_dev, const int32_t* count_dev, int32_t ncurves, int32_t max_count,
                          int32_t window, int32_t through_float32, void* stream);

/* ---- a19-a21: z-plane AR pole fit ----------------------------------------------------------------------------
 * Covariance-method AR least squares of order `order` on segments x[xoff[e] .. +len[e]) / divisor[e]
 * (divisor_dev may be NULL = 1; if x64_dev != NULL the samples are read from it as float64 instead): normal equations G = A^T A, r = A^T y with A[n,k] = s[n-k], y = -s[n],
 * n = order..len-1, contracted in float64 on the matrix cores, optional ridge added to the diagonal, Cholesky
 * solve.  coeffs_dev[e*(order+1) ..] = [1, a_1 .. a_order].  Replaces _fit_ar_least_squares, reference
 * analyse/zplane.py:83-120 (which uses an SVD-based lstsq; results agree to ~cond(A)^2 * 1e-16).
 * partial_dev: nb * ira_ar_partial_doubles(order, max_len) doubles of scratch; gscratch_dev: nb*order*order
 * doubles, only needed when order > 128; info_dev (optional): IRA_AR_INFO_DOUBLES doubles per element
 * [0] status: 0 solved, 1 a Cholesky pivot was not positive, 2 solved and refined (ira_ar_refine), 3 not finite (a NaN or
 * infinite sample: coefficients 1, NaN ..; written by ira_ar_solve itself, at every order, with or without a ridge),
 * 4 rank-deficient: minimum-norm solution (ira_ar_minnorm, which then redefines [1..3]), 5 solved by the double-double
 * normal equations (ira_ar_exact), [1] largest,
 * [2] smallest pivot, [3] condition estimate trace(G) * ||G^-1|| (two inverse iterations on the factor, started from the
 * alternating vector): at most order * cond(G); no rigorous lower bound -- on high-passed signals of even order the
 * start vector is orthogonal to the weak direction; the tests hold it above 0.25 cond(G), the smallest ratio measured
 * is recorded in tests/test_gpu_ar.py).  1 <= order <= 1024 < len. */
#define IRA_AR_INFO_DOUBLES 4
#define IRA_AR_STATUS_SOLVED 0       /* info[0], as listed above (stored as a double) */
#define IRA_AR_STATUS_PIVOT 1
#define IRA_AR_STATUS_REFINED 2
#define IRA_AR_STATUS_NOT_FINITE 3
#define IRA_AR_STATUS_MINNORM 4
#define IRA_AR_STATUS_EXACT 5
#define IRA_AR_DENSE_GRAM 1   /* flags: form G = A^T A as a dense contraction on the FP64 matrix cores (v_mfma_f64_16x16x4_f64)
                               * instead of the O(order * len) lag-sum form: the cross-check of the default path.  gram, solve
                               * and refine of one fit take the same flags (layout of partial_dev). */
#define IRA_AR_WORKGROUP_SOLVE 2   /* flags (ira_ar_solve / ira_ar_refine): the 256-thread solve kernel also for order <= 64, where one wave
                                    * per element is the default since round 4 (A/B and cross-check: both give the same bits) */
int64_t ira_ar_partial_doubles(int32_t order, int32_t max_len);
/* The two halves of ira_ar_fit, callable separately: the MFMA Gram contraction, and reduce + Cholesky solve. */
int32_t ira_ar_gram(const float* x_dev, const double* x64_dev, const int64_t* xoff_dev,
                    const int32_t* len_dev, const double* divisor_dev, int32_t nb, int32_t max_len,
                    int32_t order, double* partial_dev, int32_t flags, void* stream);
int32_t ira_ar_solve(const double* partial_dev, const int32_t* len_dev, int32_t nb, int32_t max_len,
                     int32_t order, double ridge, double* gscratch_dev, double* coeffs_dev,
                     double* info_dev, int32_t flags, void* stream);
/* Rank-deficient fits.  For the elements ira_ar_solve flagged with status 1 (a Cholesky pivot was not positive: constant
 * segments, a few taps followed by digital silence, segments shorter than ~2 order) -- every other element is left alone --
 * G is eigen-decomposed (cyclic Jacobi) and the MINIMUM-NORM solution a = -V diag(1/lambda_k | 0) V^T r is written, dropping
 * directions with lambda_k <= rel_cut * lambda_max: what numpy.linalg.lstsq(A, y, rcond=None) returns for a rank-deficient A
 * (reference analyse/zplane.py:117).  info becomes [4, lambda_max, smallest kept lambda, rank]; a Gram matrix holding NaN or
 * infinity (the reference's lstsq raises LinAlgError there) gives status 3 and NaN coefficients.  scratch2_dev: nb * 2 *
 * order^2 doubles; order <= 512; rel_cut in (0, 1), 1e-12 sits just above the rounding noise of a float64 Gram matrix.
 * Runs after ira_ar_solve (ridge = 0, default lag-sum record: not with IRA_AR_DENSE_GRAM) on the same partial / coeffs /
 * info buffers, before ira_ar_refine. */
int32_t ira_ar_minnorm(const double* partial_dev, const int32_t* len_dev, int32_t nb, int32_t max_len, int32_t order,
                       double* scratch2_dev, double* coeffs_dev, double* info_dev, double rel_cut, void* stream);
/* Ill-conditioned fits beyond the reach of refinement: elements whose float64 Cholesky broke down (status 1) or whose
 * condition estimate info[3] exceeds cond_threshold (1e13: cond(G) eps is no longer small) are solved again with the normal
 * equations carried in DOUBLE-DOUBLE arithmetic: the p+1 lag sums accumulated from exact products of the samples (two_prod +
 * compensated sums, ~106 bits), G assembled from them, Cholesky and both triangular solves in the same arithmetic.  The
 * result is good to cond(G) x 1e-32 -- better than the reference's SVD-based lstsq (zplane.py:117, ~cond(A) eps), with
 * which it agrees to 2e-9 on tests/golden/ar_illcond.npz (500 Hz low-passed float32 response, cond(G) ~ 1e17, where the
 * float64 normal equations are off by 35 %).  info[0] becomes 5; a Gram matrix singular to 1e-26 of its trace keeps status
 * 1 for ira_ar_minnorm.  Runs after ira_ar_solve, before ira_ar_minnorm / ira_ar_refine, on the same partial / coeffs / info
 * buffers (lag-sum record only: not with IRA_AR_DENSE_GRAM).  ddpartial_dev: nb * ira_ar_exact_doubles(order, max_len, 0)
 * doubles, ddscratch_dev: nb * ira_ar_exact_doubles(order, max_len, 1).  Unflagged elements cost nothing but the launches. */
int64_t ira_ar_exact_doubles(int32_t order, int32_t max_len, int32_t which);
int32_t ira_ar_exact(const float* x_dev, const double* x64_dev, const int64_t* xoff_dev, const int32_t* len_dev,
                     const double* divisor_dev, int32_t nb, int32_t max_len, int32_t order, double ridge,
                     const double* partial_dev, double* ddpartial_dev, double* ddscratch_dev, double* coeffs_dev,
                     double* info_dev, double cond_threshold, void* stream);
/* Iterative refinement for ill-conditioned fits (ridge = 0 only).  The reference's SVD-based lstsq is accurate to about
 * cond(A) eps, the normal equations only to cond(A)^2 eps = cond(G) eps; elements whose condition estimate
 * info[3] > cond_threshold get `steps` (1..4) rounds of  a += G^-1 A^T (y - A a)  with the residual and
 * its gradient formed from the samples in float64 (corrected semi-normal equations): error ~ cond(A) eps again as long
 * as cond(A)^2 eps < 1.  Runs after ira_ar_solve with the same partial/coeffs/info buffers; grad_dev: nb *
 * ceil((max_len - order) / 4096) * (order + 1) doubles of scratch.  Unflagged elements cost nothing but the launch.
 * info[0] becomes 2 for refined elements. */
int32_t ira_ar_refine(const float* x_dev, const double* x64_dev, const int64_t* xoff_dev, const int32_t* len_dev,
                      const double* divisor_dev, int32_t nb, int32_t max_len, int32_t order, const double* partial_dev,
                      double* gscratch_dev, double* coeffs_dev, double* info_dev, double* grad_dev,
                      double cond_threshold, int32_t steps, int32_t flags, void* stream);
int32_t ira_ar_fit(const float* x_dev, const double* x64_dev, const int64_t* xoff_dev,
                   const int32_t* len_dev, const double* divisor_dev, int32_t nb, int32_t max_len, int32_t order, double ridge,
                   double* partial_dev, double* gscratch_dev, double* coeffs_dev, double* info_dev,
                   int32_t flags, void* stream);

/* All complex roots of npoly real polynomials given in DESCENDING powers, ncoef coefficients each
 * (Aberth-Ehrlich, float64).  Trailing coefficients with |c| < trail_eps are dropped first (reference
 * analyse/zplane.py:153-155), then numpy.roots conventions apply (leading zeros stripped, exact trailing
 * zeros are roots at 0).  roots_dev: npoly * (ncoef-1) interleaved (re, im); nroots_dev[e] = count found.
 * Replaces _roots_from_poly_descending, reference analyse/zplane.py:145-158.  Root order is unspecified. */
int32_t ira_poly_roots(const double* coeffs_dev, int32_t npoly, int32_t ncoef, double trail_eps,
                       double* roots_dev, int32_t* nroots_dev, void* stream);

/* b[e][n] = sum_k a[e][k] * s[n-k], n = 0..zero_order.  Replaces _derive_fir_numerator_from_ar, reference
 * analyse/zplane.py:123-142. */
int32_t ira_fir_numerator(const double* coeffs_dev, int32_t order, const float* x_dev,
                          const int64_t* xoff_dev, const int32_t* len_dev, const double* divisor_dev,
                          int32_t nb, int32_t zero_order, double* b_dev, void* stream);

/* ---- Direct transforms of smooth lengths -------------------------------------------------------------------------------
 * For n = 2^a 3^b 5^c that splits as n1*n2 with both factors <= 1024 (480000 = 640*750, 2^19 = 512*1024, ...) a
 * two-pass mixed-radix four-step transform replaces the three-pass Bluestein of ira_rfft_any / ira_band_irfft; every
 * job of a call has the same length n.  ira_fft_smooth_split: IRA_OK and the split, or IRA_E_UNSUPPORTED (then use
 * the Bluestein entry points; also when IRA_NO_SMOOTH_FFT is set in the environment).  Tables for the split:
 *   t1_dev[k] = exp(-2 pi i k/n1), k < n1;  t2_dev[k] = exp(-2 pi i k/n2), k < n2;  tf_dev[k] = exp(-2 pi i k/n), k < n2.
 * work_dev: nb * n complex f64.  All other arguments mean what they mean in ira_rfft_any / ira_band_irfft (same
 * reference call sites: frequency_response.py:204-213, filterplot.py:145-152, rt60bands.py:170-175,
 * group_delay.py:95-109).
 * Half-size modes (round 3), so that a channel's transforms never share a complex transform with ANOTHER channel's signal
 * and its results cannot depend on its neighbours in a batch (byte-identical records for any sharding):
 *   ira_rfft_smooth(..., interleave = 1): every job is ONE real signal of even length 2 n carried as the n-point complex
 *     sequence x[2m] + i x[2m+1] (x2off_dev[e] = xoff_dev[e] + 1; data_len / win_len, when given, count REAL samples; the
 *     second signal's length arrays must be NULL); spec_off_dev[e] receives its n + 1 bins.  zpair: n complex per job --
 *     or NULL (round 4, n1 even): the untangling is then part of the second pass (the intermediate is laid out in tiles
 *     of a row and its mirror row, so Z[k] and Z[n-k] meet in one workgroup) and no scratch or split pass exists.
 *   ira_band_irfft_smooth(..., half_out = 1): every job is ONE band (band record 2e; record 2e+1 is ignored) of a real
 *     signal of even length 2 n, computed by an n-point transform: the job's half spectrum has n + 1 bins, y1_off_dev[e]
 *     receives 2 n samples, y2_off_dev is ignored, spec_off2_dev must be NULL.
 *   ira_band_irfft_smooth(..., job_info_dev): nb * 4 int32 of device scratch, or NULL.  With it (round 4) NARROW jobs -- the
 *     hull of the job's band supports spans at most 9 n2 bins, e.g. the third-octave bands below ~800 Hz of a 10 s file --
 *     skip the first pass and the n-point work array altogether: their few non-zero bins are compacted once per job and
 *     the second pass sums the <= 2 x 9 terms of the pruned first pass per point in its input stage.  Which jobs are narrow
 *     is decided on the device from the mask records (job_info_dev[4e .. 4e+3] = {narrow, first bin, bins, terms}, an
 *     output for the curious).  Same results up to float64 rounding of a different summation order; NULL = every job
 *     takes both passes.
 *   ira_band_irfft_smooth(..., tile_part_dev) (round 5; may be NULL): the second pass also leaves the ENERGIES of the
 *     4096-sample tiles (counted from the end of each band signal) of what it writes, as partial sums per workgroup:
 *     job e, signal s (0: y1, 1: y2; a half_out job has signal 0 only), tile j, workgroup w at
 *     tile_part_dev[((e * 2 + s) * workgroups + w) * tiles + j], with (tiles, workgroups) = ira_band_tile_layout(n, half_out):
 *     nb * 2 * tiles * workgroups doubles.  ira_edc_fits(tile_part_dev ...) turns them into its tile totals and no longer
 *     reads every band signal twice (reference rt60bands.py:170-175 -> :272-321). */
int32_t ira_fft_smooth_split(int32_t n, int32_t* n1, int32_t* n2);
int32_t ira_band_tile_layout(int32_t n, int32_t half_out, int32_t* tiles, int32_t* workgroups);
int32_t ira_rfft_smooth(const float* x_dev, const int64_t* xoff_dev, int32_t n, int32_t nb, int32_t use_hann,
                        const void* t1_dev, const void* t2_dev, const void* tf_dev, double* work_dev,
                        double* spec_out_dev, const int64_t* spec_off_dev, const int64_t* x2off_dev,
                        const int64_t* spec_off2_dev, double* zpair_dev, const int64_t* zpair_off_dev,
                        const int32_t* data_len_dev, const int32_t* win_len_dev, const int32_t* data_len2_dev,
                        const int32_t* win_len2_dev, int32_t interleave, void* stream);
int32_t ira_band_irfft_smooth(const double* spec_dev, const int64_t* spec_off_dev, int32_t n, int32_t nb,
                              const double* band_params_dev, const double* freq_val_dev, const void* t1_dev,
                              const void* t2_dev, const void* tf_dev, double* work_dev, float* y_dev,
                              const int64_t* y1_off_dev, const int64_t* y2_off_dev, const int64_t* spec_off2_dev,
                              int32_t half_out, int32_t* job_info_dev, double* tile_part_dev, void* stream);

/* k-th smallest values (0-based ranks, clipped to the segment) of float64 segments values_dev + off_dev[e], count_dev[e]
 * long: out_dev[e*nranks + j] = sorted(segment)[ranks_dev[e*nranks + j]], 1 <= nranks <= 8 (radix select, exact).
 * The building block of numpy.median / numpy.percentile in summarise_group_delay_results_text, reference
 * analyse/group_delay.py:209-220 (the interpolation between neighbouring ranks stays on the host). */
int32_t ira_order_stats(const double* values_dev, const int64_t* off_dev, const int32_t* count_dev, int32_t nseg,
                        const int64_t* ranks_dev, int32_t nranks, double* out_dev, void* stream);

/* ---- Section 8f: diffusion / decorrelation per time window ----------------------------------------------------------
 * Element e: float32 signal at x_dev + xoff_dev[e] (already trimmed), nframes_dev[e] windows of `win` samples every
 * `hop` (16 <= win <= 8192, 1 <= max_lag <= 4096).  Per window, with w0 = w - mean(w) in float32 exactly as numpy
 * computes it (pairwise float32 sum):
 *   ac[e][f] = max_{lag=1..min(max_lag, win-2)} |sum_k w0[k] w0[k+lag]| / sum w0^2     (NaN if the energy <= 1e-20)
 *   ed[e][f] = fraction(|w0| > float32(thr_rms * rms)) [/ gauss_expected if gauss_expected >= 0], rms = float32
 *              sqrt(mean(w0*w0));  NaN if rms <= 1e-20 or 0 <= gauss_expected <= 1e-12.
 * Outputs float32 at out_off_dev[e] + f.  Replaces _windowed_max_abs_autocorr / _windowed_echo_density and the frame
 * loop of analyse_diffusion_for_channel, reference analyse/diffusion.py:139-159, :205-226, :264-276. */
int32_t ira_diffusion(const float* x_dev, const int64_t* xoff_dev, const int32_t* nframes_dev, int32_t nb,
                      int32_t max_frames, int32_t win, int32_t hop, int32_t max_lag, double thr_rms,
                      double gauss_expected, float* ac_dev, float* ed_dev, const int64_t* out_off_dev,
                      void* stream);

/* Stereo pair per element (left at loff_dev[e], right at roff_dev[e], same geometry): zero-lag Pearson correlation
 * and max |normalised cross-correlation| over lags -max_lag..+max_lag per window.  Replaces _windowed_corr0 /
 * _windowed_iacc_max and the frame loop of reference analyse/diffusion.py:162-202, :346-358. */
int32_t ira_diffusion_stereo(const float* x_dev, const int64_t* loff_dev, const int64_t* roff_dev,
                             const int32_t* nframes_dev, int32_t nb, int32_t max_frames, int32_t win, int32_t hop,
                             int32_t max_lag, float* corr0_dev, float* iacc_dev, const int64_t* out_off_dev,
                             void* stream);

/* ---- Section 8f, rank 2: native tap ingest (RIFF/WAVE 16-bit PCM as written by the reference's C++ recorder,
 * include/analysis/recorder.hpp:55-90) ----------------------------------------------------------------------------
 * ira_wav_probe: HOST call; walks the RIFF chunks of `path` and reports rate / channels / frames and the byte offset
 *   of the sample data.  IRA_OK for mono/stereo PCM16, IRA_E_UNSUPPORTED for any other valid WAV encoding (use the
 *   Python reader), IRA_E_IO if the file cannot be opened or is shorter than
 *   its header says, IRA_E_FORMAT if it is not RIFF/WAVE (scipy.io.wavfile.read raises FileNotFoundError / ValueError there).
 * ira_wav_read_pcm16: HOST call; reads frames*channels interleaved int16 into dst_host (ideally pinned memory).
 * ira_pcm16_to_channels: DEVICE; interleaved int16 -> planar float32 channels (out[c*frames + i]) with the
 *   reference's conversion x/32768 clipped to [-1, 1] (analyse/io.py:46-64, :98-113), or with mono_downmix (stereo
 *   only) the single channel 0.5*(L+R) in float32 (analyse/io.py:85-91).  Replaces scipy.io.wavfile.read +
 *   convert_wav_samples_to_float32 + get_analysis_channels for tap files; the upload carries 2 bytes per sample. */
int32_t ira_wav_probe(const char* path, int32_t* sample_rate, int32_t* channels, int64_t* frames,
                      int64_t* data_offset);
int32_t ira_wav_read_pcm16(const char* path, int64_t data_offset, int64_t frames, int32_t channels,
                           int16_t* dst_host);

/* The same for a whole group of files in ONE call, on `threads` host threads created and joined inside the call (a caller
 * with an interpreter lock releases it once per group instead of once per file).  status[i] = what ira_wav_probe /
 * ira_wav_read_pcm16 returns for file i; the return value is IRA_OK unless an argument is NULL / n < 0.  File i's payload
 * goes to dst_host + dst_off[i] (int16 elements).  Replaces the per-file loop around scipy.io.wavfile.read of reference
 * analyse/bundle.py:56-67 -> report.py -> io.py:200. */
int32_t ira_wav_probe_batch(const char* const* paths, int32_t n, int32_t threads, int32_t* status, int32_t* sample_rate,
                            int32_t* channels, int64_t* frames, int64_t* data_offset);
int32_t ira_wav_read_pcm16_batch(const char* const* paths, const int64_t* data_offset, const int64_t* frames,
                                 const int32_t* channels, const int64_t* dst_off, int16_t* dst_host, int32_t n,
                                 int32_t threads, int32_t* status);
int32_t ira_pcm16_to_channels(const int16_t* pcm_dev, int64_t frames, int32_t channels, int32_t mono_downmix,
                              float* out_dev, void* stream);
/* The same conversion for a GROUP of tap files in one launch (a bundle step holds 32 taps; one launch per tap was 27 % of a
 * step's device time).  File f: interleaved int16 at pcm_dev + src_off[f] (even element offset: 4-byte frame loads),
 * frames[f] frames of channels[f] in {1, 2} channels, mode[f] 1 = stereo mixed down to 0.5 * (L + R) in float32 (reference
 * analyse/io.py:85-91), 0 = planar channels; output at out_dev + dst_off[f] (channel c at + c * frames[f]).  max_frames >=
 * every frames[f] sizes the grid.  Replaces the per-file loop over scipy.io.wavfile.read + convert_wav_samples_to_float32
 * + get_analysis_channels of reference analyse/io.py:46-113, :181-221 for a whole group. */
int32_t ira_pcm16_to_channels_jobs(const int16_t* pcm_dev, const int64_t* src_off_dev, const int64_t* frames_dev,
                                   const int32_t* channels_dev, const int32_t* mode_dev, const int64_t* dst_off_dev,
                                   int32_t nfiles, int64_t max_frames, float* out_dev, void* stream);

/* ---- a8 alone: mask_dev[k] = the float32 mask value the band inverses multiply bin k with, k < nbins, for ONE band record
 * (band_params8: HOST array of 8 doubles, as in ira_band_irfft) on the axis float32(k * freq_val).  The reference's
 * _make_lowpass_mask / _make_highpass_mask / _make_bandpass_mask (analyse/rt60bands.py:116-167) evaluated by the very
 * device function the transforms inline -- for tests and for callers that want the mask itself. */
int32_t ira_band_mask_values(const double* band_params8, double freq_val, int64_t nbins, float* mask_dev, void* stream);

/* ira_host_pull: DEVICE kernel that reads PINNED (mapped) host memory over the PCIe link and writes HBM -- the batch upload
 *   without the copy engine, and for PCM16 with the conversion of io.py:46-64 (x/32768 clipped) in the same pass (no int16
 *   staging buffer in HBM).  host_src: host pointer of a pinned allocation (hipHostMalloc / torch pin_memory), 16-byte
 *   aligned; count samples; format 0 = float32 copied as is, 1 = mono int16 -> float32; out_dev 16-byte aligned;
 *   workgroups = grid size (0 = 8: just enough reads in flight to fill a Gen5 x16 link; more only crowd the fabric queues
 *   the analysis kernels' HBM reads go through).  Throughput equals hipMemcpyAsync's within noise: an
 *   option, not the default.  IRA_E_UNSUPPORTED if host_src is not mapped host memory. */
int32_t ira_host_pull(const void* host_src, int64_t count, int32_t format, float* out_dev, int32_t workgroups,
                      void* stream);

/* ---- Section 8f, rank 4: sweep deconvolution (reference analyse/deconvolve.py:124-193) -----------------------------------
 * The transforms are ira_rfft_any / ira_rfft_smooth (zero-padded to n_fft = next power of two, no window) and
 * ira_band_irfft / ira_band_irfft_smooth (all-pass mask).  In between and after:
 * ira_deconv_divide: element e: Y (half spectrum of nfft[e]/2+1 bins at yspec_dev + 2*yspec_off[e], overwritten) becomes
 *   H = Y conj(X) / (|X|^2 + eps) with X at xspec_dev + 2*xspec_off[e] (elements may share one sweep spectrum) and
 *   eps = regularization_relative * max(1e-30, max_k |X_k|^2), |X|^2 formed as hypot(re, im)^2 like numpy.abs(X)**2
 *   (deconvolve.py:150-166).  pmax_dev: nb doubles of scratch (receives max |X|^2 per element).
 * ira_deconv_finish: element e is one channel of length n_out[e] at h_dev + h_off[e], group[e] < ngroups its FILE:
 *   remove_dc: h -= float32(mean(h)) per channel; normalise_peak: every channel of a file is multiplied by
 *   float32(target_peak / max |h| over the file) unless that peak is 0; the peak is numpy.max(numpy.abs(.)), so a NaN
 *   sample in any channel of a file makes every sample of the file NaN (deconvolve.py:176-189, :100-106).  mean_dev: nb
 *   floats, peak_bits_dev: ngroups uint32 of scratch. */
int32_t ira_deconv_divide(double* yspec_dev, const int64_t* yspec_off_dev, const double* xspec_dev,
                          const int64_t* xspec_off_dev, const int32_t* nfft_dev, int32_t nb, int32_t max_nfft,
                          double regularization_relative, double* pmax_dev, void* stream);
int32_t ira_deconv_finish(float* h_dev, const int64_t* h_off_dev, const int32_t* n_out_dev, const int32_t* group_dev,
                          int32_t nb, int32_t ngroups, int32_t max_len, int32_t remove_dc, int32_t normalise_peak,
                          double target_peak, float* mean_dev, uint32_t* peak_bits_dev, void* stream);

/* ---- ISO 3382-1 energy-ratio parameters: clarity C_k, definition D, centre time Ts ----------------------------------
 * Nothing in the reference computes these (it reports decay times only); they replace no reference function.  Host side:
 * audio_analysis_amd/analyse/energy.py (`python -m analyse.energy`).
 * ira_onset_index: onset_dev[s] = the smallest n <= p with float64(x[n])^2 >= float64(x[p])^2 * rel_energy (float64
 *   compare), p = peak_dev[s] as ira_peak_index wrote it and peak_abs_dev[s] = |x[p]| -- read on the device, no host round
 *   trip (ISO 3382-1 A.3.4: the first point within 20 dB of the maximum is rel_energy = 10^(-20/10)).  rel_energy in
 *   [0, 1]; max_len = longest segment (sizes the grid; < 2^32); nseg <= 65535.  Exact integer result.
 * ira_energy_windows: segment j = base_len[j] - o samples from base_off[j] + o, o = onset_dev[chan_of_seg[j]] (band signals
 *   of a channel share its broadband onset).  With the segment's nlim (1..4) ascending sample limits
 *   limits_dev[j * nlim + k] (per segment: channels of different sample rates share a launch), out_dev[j * (nlim + 2) + i]:
 *   i <= nlim: P_i = sum of float64(x)^2 over [N_i, N_{i+1}) (N_0 = 0, N_{nlim+1} = segment length), i = nlim + 1:
 *   S1 = sum n x[n]^2.  Float64 sums in an order that depends on the segment alone (bit-identical whatever the batch, the
 *   segment's place in it or its alignment).  max_len >= every base_len (< 2^31); nseg <= 65535; scratch_dev holds
 *   ira_energy_scratch_doubles(nseg, max_len, nlim) doubles (IRA_E_SIZE, negative, for arguments out of range). */
int32_t ira_onset_index(const float* x_dev, const int64_t* off_dev, const int64_t* len_dev, int32_t nseg, int64_t max_len,
                        const int64_t* peak_dev, const float* peak_abs_dev, double rel_energy, int64_t* onset_dev,
                        void* stream);
int64_t ira_energy_scratch_doubles(int32_t nseg, int64_t max_len, int32_t nlim);
int32_t ira_energy_windows(const float* x_dev, const int64_t* base_off_dev, const int64_t* base_len_dev,
                           const int32_t* chan_of_seg_dev, const int64_t* onset_dev, int32_t nseg, int64_t max_len,
                           const int64_t* limits_dev, int32_t nlim, double* scratch_dev, double* out_dev, void* stream);

/* ---- ISO 3382-1 Annex B inter-channel cross-correlation: IACC_E, IACC_L, IACC_A -------------------------------------
 * Nothing in the reference computes these (its only two-channel quantity is the short-time series of the diffusion
 * block); both entry points replace no reference function.  Host side: audio_analysis_amd/analyse/iacc.py
 * (`python -m analyse.iacc`).
 * ira_xcorr_windows: segment j is one signal row of a stereo pair: left channel len_dev[j] samples at x_dev + l_off_dev[j],
 *   right channel as many at x_dev + r_off_dev[j].  o = min(onset_dev[lchan_of_seg_dev[j]], onset_dev[rchan_of_seg_dev[j]])
 *   is taken on the device (band rows of a pair share its broadband onsets), L = len - o, n counts from o.  With the
 *   segment's nlim (1..4) ascending sample limits limits_dev[j * nlim + k] the partitions are [0, N_1), ..., [N_nlim, L),
 *   and out_dev[(j * (nlim + 1) + i) * (2 T + 3) + ...] holds for partition i, T = max_lag (1..IRA_XCORR_MAX_LAG):
 *     C(tau) = sum_n l[o + n] r[o + n + tau], tau = -T .. T in this order (r = 0 outside the file: the right channel is read
 *     across partition boundaries and in front of the onset, never wrapped), then El = sum_n l[o + n]^2, Er = sum_n r[o + n]^2.
 *   Float64 products and sums of the exact float32 samples, in an order that depends on the segment's length, onset and
 *   limits alone (bit-identical whatever the batch, the segment's place in it or its alignment); no atomics.
 *   Every limit is clamped to 0 .. L and an upper limit below its partition's lower one gives an empty partition (zeros),
 *   as does every partition of a segment whose o is negative or past its len.  A len above max_len is a caller's error that
 *   stays inside the scratch: such a segment comes out cut at the ceil(max_len / 4096) chunks of 4096 rows (counted from o)
 *   that its records were sized for, like a row of ira_mtf_sums.
 *   max_len >= every len (< 2^31); nseg <= 65535; scratch_dev holds as many doubles as the size call returns
 *   (IRA_E_SIZE, negative, for arguments out of range; the size call is host only).  Argument errors are reported
 *   before anything is launched. */
#define IRA_XCORR_MAX_LAG 128
int64_t ira_xcorr_scratch_doubles(int32_t nseg, int64_t max_len, int32_t nlim, int32_t max_lag);
int32_t ira_xcorr_windows(const float* x_dev, const int64_t* l_off_dev, const int64_t* r_off_dev, const int64_t* len_dev,
                          const int32_t* lchan_of_seg_dev, const int32_t* rchan_of_seg_dev, const int64_t* onset_dev,
                          int32_t nseg, int64_t max_len, const int64_t* limits_dev, int32_t nlim, int32_t max_lag,
                          double* scratch_dev, double* out_dev, void* stream);

/* ---- ISO 3382-1 noise handling: Lundeby cross-point, truncated and compensated Schroeder integration ------------------
 * Nothing in the reference estimates a noise floor (its decay fits integrate to the last sample of the file); the four
 * entry points below replace no reference function.  Host side and the algorithm they carry out, step by step:
 * audio_analysis_amd/analyse/lundeby.py (`python -m analyse.lundeby`).
 * Rows: row j is base_len[j] - s samples from x_dev + base_off[j] + s, s = start_dev[chan_of_seg[j]] read on the device (the
 *   band rows of a channel share its broadband start index), L = base_len[j] - s.  blk_size_dev[j] = B (1..4096) and
 *   nblk_dev[j] = nb (<= IRA_LUNDEBY_MAX_BLOCKS) are the host's; a row whose nb != L / B, or whose L exceeds 2047 * 4096
 *   samples, is treated as a row without blocks (status IRA_LUNDEBY_TOO_SHORT), never read out of bounds.  The row's table
 *   of nb + 1 doubles lies at blk_off_dev[j] of blk_dev and of suffix_dev (ira_lundeby_scratch_doubles(nseg, max nb) doubles
 *   each hold every row at a stride of max nb + 1; IRA_E_SIZE, negative, for arguments out of range; host only).
 *   max_chunks >= ceil((nb + 1) / (4096 / B)) for every row sizes the grids of the two sample passes.  nseg <= 65535.
 *   Argument errors are reported before anything is launched.  Float64 sums in an order that depends on the row's own B and
 *   L alone: results are bit-identical whatever the batch, the row's place in it or its alignment; no atomics.
 * ira_block_energy: blk[j] = sum of float64(y)^2 over block j < nb; blk[nb] = the same over the partial tail block (0 if
 *   there is none).
 * ira_lundeby_estimate: steps 2 to 6 of the algorithm; first_m_dev[j] = m0 (intervals of the preliminary pass, in blocks);
 *   compensate = 1 adds the compensation energy C, 0 truncates only.  rec_dev: IRA_LUNDEBY_DOUBLES doubles per row:
 *     [0] status (IRA_LUNDEBY_* bits) [1] Ln dB [2] t1 samples [3] slope dB per sample [4] intercept dB [5] C
 *     [6] rounds [7] m1 [8] kmax [9] k0 [10] k1 [11] preliminary cross-point [12] final cross-point (samples) [13] max M
 *     [14] edc[0] (energy, C included) [15] blocks the curve covers;  [1..15] are NaN on an error status (bits 1 to 16).
 *   len_out_dev[j] (int64): samples of the curve: t1; L with IRA_LUNDEBY_NO_FLOOR; 0 on an error status.
 *   suffix_dev: per block of the curve the energy behind it inside the curve, plus C.
 * ira_edc_truncated: edc[i] = (reverse sum inside i's block) + suffix[block] for i < len_dev[j] (edc[0] is rec[14] to
 *   the bit), then the chain of ira_edc_db: max(., eps) / max(edc[0], eps) -> 10 log10 -> max(., floor_db) -> float32 at
 *   edc_dev + edc_off_dev[j].  Nothing is written at or after len_dev[j].  A row may be written over its own samples
 *   (edc_dev + edc_off_dev[j] == x_dev + base_off[j] + s). */
#define IRA_LUNDEBY_DOUBLES 16
#define IRA_LUNDEBY_MAX_BLOCKS 4096
#define IRA_LUNDEBY_SILENT 1
#define IRA_LUNDEBY_TOO_SHORT 2
#define IRA_LUNDEBY_NO_RANGE 4
#define IRA_LUNDEBY_SLOPE 8
#define IRA_LUNDEBY_NON_FINITE 16
#define IRA_LUNDEBY_NO_FLOOR 32
int64_t ira_lundeby_scratch_doubles(int32_t nseg, int32_t max_nblk);
int32_t ira_block_energy(const float* x_dev, const int64_t* base_off_dev, const int64_t* base_len_dev,
                         const int32_t* chan_of_seg_dev, const int64_t* start_dev, const int32_t* blk_size_dev,
                         const int32_t* nblk_dev, const int64_t* blk_off_dev, int32_t nseg, int32_t max_chunks,
                         double* blk_dev, void* stream);
int32_t ira_lundeby_estimate(const int64_t* base_len_dev, const int32_t* chan_of_seg_dev, const int64_t* start_dev,
                             const int32_t* blk_size_dev, const int32_t* nblk_dev, const int32_t* first_m_dev,
                             const int64_t* blk_off_dev, int32_t nseg, const double* blk_dev, int32_t compensate,
                             double* rec_dev, int64_t* len_out_dev, double* suffix_dev, void* stream);
int32_t ira_edc_truncated(const float* x_dev, const int64_t* base_off_dev, const int64_t* base_len_dev,
                          const int32_t* chan_of_seg_dev, const int64_t* start_dev, const int32_t* blk_size_dev,
                          const int32_t* nblk_dev, const int64_t* blk_off_dev, int32_t nseg, int32_t max_chunks,
                          const double* rec_dev, const int64_t* len_dev, const double* suffix_dev, double eps,
                          double floor_db, float* edc_dev, const int64_t* edc_off_dev, void* stream);

/* ---- Multi-slope decay fits (coupled rooms): sums of exponentials plus a noise term on the Schroeder curve -------------
 * Nothing in the reference fits more than one slope; the three entry points below replace no reference function.  Host
 * side and the algorithm they carry out, step by step: audio_analysis_amd/analyse/multislope.py
 * (`python -m analyse.multislope`).  Rows and their tables (base_len .. blk_off, nseg <= 65535) are those of
 * ira_block_energy, whose output blk_dev is the input here.  Float64 throughout, no atomics, every sum in an order that
 * depends on the row alone: a row's records are bit-identical whatever the batch, its place in it or its alignment.
 * Argument errors (IRA_E_NULL / IRA_E_SIZE) are reported before anything is launched; nseg = 0 or njobs = 0: IRA_OK.
 * ira_multislope_points: d[j] = tail + E[nb - 1] + .. + E[j] for j < nb at blk_off_dev[row] of d_dev (laid out like
 *   blk_dev; untouched on an error status); info_dev[2 row] = the row status (IRA_MS_SILENT .. IRA_MS_NON_FINITE, checked in
 *   the order too short, non-finite, silent, zero in range), info_dev[2 row + 1] = J = max(1, floor(fit_fraction nb)), the
 *   product rounded to float64, 0 < fit_fraction <= 1.  rec_dev: IRA_MS_MAX_ORDER records of IRA_MS_DOUBLES doubles per
 *   row, written here as [0] status [1] J [14] d[0] and NaN elsewhere ([1] and [14] NaN too on an error status).
 *   Rows with an error status are skipped by the two kernels below.
 * ira_multislope_gram: job i = job_dev[3 i ..] = (row, grid slot, Gram slot).  Grid slot k holds grid_n_dev[k] <= max_g
 *   ascending decay times in seconds at grid_dev + k grid_stride (grid_stride >= max_g, max_g <= IRA_MS_MAX_GRID).  With
 *   g = the grid's size, functions 0 .. g - 1 the decays, g the noise term and g + 1 the constant 1, the Gram slot
 *   (gram_dev + slot (max_g + 2)(max_g + 3) / 2) receives the lower triangle out[i (i + 1) / 2 + k], k <= i <= g + 1, of
 *   sum_j u_i[j] u_k[j] over the J points: b is row g + 1.  Points are added in ascending j, IRA_MS_TILE of them staged
 *   at a time.  Entries of job_dev outside [0, nseg), [0, ngrids), [0, nslots) are skipped.
 * ira_multislope_search: job i = job_dev[4 i ..] = (row, order S in 1..IRA_MS_MAX_ORDER, Gram slot, grid slot): every
 *   candidate of order S on that grid, with and without the noise term; min_ratio > 1.  The record of (row, S), at
 *   rec_dev + (row IRA_MS_MAX_ORDER + S - 1) IRA_MS_DOUBLES:
 *     [0] 0, or IRA_MS_NO_CANDIDATE (then only [0] and [15] are written) [1] J [2] 1 with the noise term, 0 without
 *     [3] cost c [4..6] grid indices (-1 unused) [7..9] T_s seconds (NaN unused) [10..12] a_s (NaN unused) [13] a_nu (0
 *     without the noise term) [14] d[0] [15] g.
 *   refine_step > 0: the next level's grid, the ascending union of T_s exp(k refine_step), k = -IRA_MS_REFINE_R ..
 *   IRA_MS_REFINE_R (equal values once), goes to grid_out_dev + (row IRA_MS_MAX_ORDER + S - 1) IRA_MS_REFINED, its size to
 *   grid_n_out_dev at the same index (0 without a candidate); refine_step = 0: neither is touched (both may be NULL). */
#define IRA_MS_DOUBLES 16
#define IRA_MS_MAX_GRID 128
#define IRA_MS_MAX_ORDER 3
#define IRA_MS_TILE 32
#define IRA_MS_REFINE_R 3
#define IRA_MS_REFINED 21
#define IRA_MS_SILENT 1
#define IRA_MS_TOO_SHORT 2
#define IRA_MS_ZERO_IN_RANGE 4
#define IRA_MS_NON_FINITE 16
#define IRA_MS_NO_CANDIDATE 32
int32_t ira_multislope_points(const int64_t* base_len_dev, const int32_t* chan_of_seg_dev, const int64_t* start_dev,
                              const int32_t* blk_size_dev, const int32_t* nblk_dev, const int64_t* blk_off_dev,
                              int32_t nseg, const double* blk_dev, double fit_fraction, double* d_dev, int32_t* info_dev,
                              double* rec_dev, void* stream);
int32_t ira_multislope_gram(const int64_t* base_len_dev, const int32_t* chan_of_seg_dev, const int64_t* start_dev,
                            const int32_t* blk_size_dev, const int32_t* nblk_dev, const int64_t* blk_off_dev, int32_t nseg,
                            const double* d_dev, const int32_t* info_dev, const int32_t* job_dev, int32_t njobs,
                            const double* grid_dev, const int32_t* grid_n_dev, int32_t grid_stride, int32_t ngrids,
                            int32_t max_g, double sample_rate_hz, int32_t nslots, double* gram_dev, void* stream);
int32_t ira_multislope_search(int32_t nseg, const int32_t* info_dev, const int32_t* job_dev, int32_t njobs,
                              const double* grid_dev, const int32_t* grid_n_dev, int32_t grid_stride, int32_t ngrids,
                              int32_t max_g, const double* gram_dev, int32_t nslots, double min_ratio, double refine_step,
                              double* grid_out_dev, int32_t* grid_n_out_dev, double* rec_dev, void* stream);

/* ---- IEC 60268-16 speech transmission index: modulation transfer sums of the squared response -----------------------
 * Nothing in the reference computes a modulation transfer function or an STI; both entry points replace nothing in the
 * reference.  Host side, with the definitions pinned: audio_analysis_amd/analyse/sti.py (`python -m analyse.sti`).
 * ira_mtf_sums: row j is len_dev[j] samples at x_dev + off_dev[j]; with e[n] = float64(x[n])^2 and the row's nf
 *   (1..IRA_MTF_MAX_FREQS) modulation frequencies w_dev[j * nf + i] in turns per sample, 0 <= w <= 0.5 (per row: rows
 *   of different sample rates share a launch), out_dev[j * (2 nf + 1) + ...] holds
 *     E = sum e[n], then per frequency A_i = sum e[n] cos(2 pi frac(w_i n)), B_i = sum e[n] sin(2 pi frac(w_i n)),
 *   n counted from the row's first sample.  w n is reduced to a fraction of a turn (its low part recovered by an FMA)
 *   before any trigonometric evaluation, and every sample's phasor is the product of three directly evaluated unit
 *   phasors: no recurrence grows with the row.  Float64 sums in an order that depends on the row's length alone
 *   (bit-identical whatever the batch, the row's place in it or its alignment), one record per chunk of IRA_MTF_CHUNK
 *   samples folded in a fixed order; no atomics.  max_len >= every len (<= 2^31); nseg <= 65535; scratch_dev holds as
 *   many doubles as the size call returns (IRA_E_SIZE, negative, for arguments out of range; the size call is host
 *   only).  Argument errors are reported before anything is launched. */
#define IRA_MTF_MAX_FREQS 16
#define IRA_MTF_CHUNK 16384
int64_t ira_mtf_scratch_doubles(int32_t nseg, int64_t max_len, int32_t nf);
int32_t ira_mtf_sums(const float* x_dev, const int64_t* off_dev, const int64_t* len_dev, const double* w_dev, int32_t nseg,
                     int64_t max_len, int32_t nf, double* scratch_dev, double* out_dev, void* stream);

/* ---- Harmonic distortion from a deconvolved logarithmic sweep: harmonic windows and their band powers -----------------
 * Nothing in the reference reads the harmonic impulses its sweep deconvolution produces; both entry points replace nothing
 * in the reference.  Host side, with the definitions pinned: audio_analysis_amd/analyse/harmonics.py
 * (`python -m analyse.harmonics`).
 * ira_harmonic_windows: channel c is the circular response of nfft_dev[c] float32 samples at h_dev + h_off_dev[c], p =
 *   peak_dev[c] its linear peak as ira_peak_index wrote it (read on the device, no host round trip).  With the nharm
 *   (1..IRA_HARMONIC_MAX) lags lag_dev[k] in samples and the float64 window window_dev[0 .. seg), row r = c * nharm + k is
 *     out_dev[r * seg + i] = float32(float64(h_c[(p - lag[k] - guard + i) mod nfft_c]) * window[i]),  i < seg:
 *   one float64 product, one rounding (bit-identical with NumPy).  Every index is reduced into the channel's buffer before
 *   it is used, whatever the tables hold; a channel with nfft <= 0 gives rows of zeros.  1 <= guard < seg <= 2^21;
 *   nch * nharm <= 65535.
 * ira_harmonic_band_powers: row r is a half spectrum of nbins complex float64 values at spec_dev + 2 * spec_off_dev[r]
 *   (offsets in complex values, as ira_rfft_any leaves them), k = r % nharm its harmonic.  With the tables lo_dev / cnt_dev
 *   (nharm x nband, int32, shared by every channel), out_dev[r * nband + j] = the mean of re^2 + im^2 over the bins
 *   lo[k][j] .. lo[k][j] + cnt[k][j] - 1; exactly 0 where cnt <= 0; NaN, without reading, where the bins leave [0, nbins).
 *   One wave per band, float64 sums in an order that depends on the band's cnt alone (bit-identical whatever the batch or
 *   the row's place in it); no atomics.  nrow a multiple of nharm, <= 65535; nband 1..4096; nbins 1..2^20 + 1.
 * Neither needs scratch.  Argument errors are reported before anything is launched. */
#define IRA_HARMONIC_MAX 10
int32_t ira_harmonic_windows(const float* h_dev, const int64_t* h_off_dev, const int32_t* nfft_dev, const int64_t* peak_dev,
                             const int64_t* lag_dev, const double* window_dev, int32_t nch, int32_t nharm, int32_t guard,
                             int32_t seg, float* out_dev, void* stream);
int32_t ira_harmonic_band_powers(const double* spec_dev, const int64_t* spec_off_dev, const int32_t* lo_dev,
                                 const int32_t* cnt_dev, int32_t nrow, int32_t nharm, int32_t nband, int32_t nbins,
                                 double* out_dev, void* stream);

/* ---- Dietsch-Kraak echo criterion EK: running centre time of |p|^n, lagged difference, maximum, crossings, curve -------
 * Nothing in the reference computes an echo criterion; both entry points replace no reference function.  Host side, with
 * the definition pinned: audio_analysis_amd/analyse/echo.py (`python -m analyse.echo`).
 * ira_echo_criterion: segment j is one (channel, criterion) row: the float32 samples at x_dev + base_off_dev[j] + o, o =
 *   onset_dev[chan_of_seg_dev[j]] read on the device (band rows of a channel share its broadband onset; no host round
 *   trip), L = base_len_dev[j] - o, m counted from o.  Its parameter set is row p = param_of_seg_dev[j] of the HOST array
 *   params (nparam rows, 1..IRA_ECHO_MAX_PARAMS, of IRA_ECHO_PARAM_DOUBLES doubles; a host array so that its values are
 *   checked before anything is launched; rows of different sample rates are different sets):
 *     [0] exponent n (finite, > 0)  [1] D samples (1..IRA_ECHO_MAX_LAG)  [2] G samples (>= 0)  [3] Mmax (0..2^31)
 *     [4] S, samples per curve step (0: no curve for these rows)  [5] threshold_10  [6] threshold_50 (finite)
 *     [7] fs in Hz (finite, > 0).  [1]..[4] are whole numbers.
 *   With s[m] = float64(|y[m]|)^n (fabs for n = 1, a product for 2, sqrt for 0.5, pow otherwise; 0 for a zero sample),
 *   W[m] = s[0] + .. + s[m], V[m] = 0 s[0] + .. + m s[m], ts[m] = V[m] / (fs W[m]) (0 where W[m] = 0 and for m < 0),
 *   EK[m] = (ts[m] - ts[m - D]) / (D / fs) for m < M = min(L - G, Mmax), formed on the device from the onset,
 *   rec_dev[j * IRA_ECHO_DOUBLES + ..] = [0] max EK  [1] the first index of the maximum  [2] the first m with EK >=
 *   threshold_10, -1 for none  [3] the same for threshold_50  [4] ts[M - 1]  [5] W[M - 1]  [6] M (as defined: it may be
 *   <= 0)  [7] V[M - 1];  with M <= 0: [NaN, -1, -1, -1, NaN, 0, M, 0].
 *   ncurve > 0: curve_dev[j * ncurve + k] = float32(max EK[k S .. min((k + 1) S, M) - 1]), NaN for k S >= M and in rows
 *   with S = 0.  ncurve = 0: no curve, curve_dev may be NULL.
 *   Nothing at or after sample M of a row is read.  Float64 sums in chunks of IRA_ECHO_CHUNK samples counted from the
 *   onset, in an order that depends on the row's own onset, length and parameters alone; the only atomics are an
 *   integer minimum (first crossings) and an integer maximum (curve), which do not depend on arrival order: a row's
 *   record and curve are bit-identical whatever the batch, the row's place in it or its alignment.
 *   max_len >= every row's M (it sizes the grid and the scratch; <= 2^31); nseg <= 65535; scratch_dev holds as many
 *   doubles as the size call returns for (nseg, max_len) (IRA_E_SIZE, negative, for arguments out of range; host only).
 *   stash_dev: NULL, and the second sample pass forms s again from the samples; or nseg * ceil(max_len /
 *   IRA_ECHO_CHUNK) * IRA_ECHO_CHUNK doubles, and the first pass leaves s there for the second to read back (same
 *   results to the bit; DESIGN.md 4.12 has both times).  Argument errors are reported before anything is launched. */
#define IRA_ECHO_DOUBLES 8
#define IRA_ECHO_CHUNK 4096
#define IRA_ECHO_MAX_LAG 2048      /* halo capacity: 14 ms at 96 kHz is 1344 samples */
#define IRA_ECHO_MAX_PARAMS 16
#define IRA_ECHO_PARAM_DOUBLES 8
int64_t ira_echo_scratch_doubles(int32_t nseg, int64_t max_len);
int32_t ira_echo_criterion(const float* x_dev, const int64_t* base_off_dev, const int64_t* base_len_dev,
                           const int32_t* chan_of_seg_dev, const int32_t* param_of_seg_dev, const int64_t* onset_dev,
                           int32_t nseg, int64_t max_len, const double* params, int32_t nparam, int64_t ncurve,
                           double* scratch_dev, double* stash_dev, double* rec_dev, float* curve_dev, void* stream);

/* ---- Dual-channel spectral sums (Welch): auto- and cross-spectra over overlapping frames, H1 / H2, coherence -----------
 * Nothing in the reference computes a transfer function from two channels; both entry points replace no reference
 * function.  Host side, with the definitions pinned: audio_analysis_amd/analyse/transfer.py (`python -m
 * analyse.transfer`).
 * Pair p: reference x' = x_dev + x_off_dev[p], measurement y' = x_dev + y_off_dev[p] (float32; the pair's delay is
 *   already in the two offsets), n_dev[p] samples of each.  n_fft a power of two 256 .. 8192, 1 <= hop <= n_fft,
 *   K = 1 + (n_dev[p] - n_fft) / hop frames (0 when n_dev[p] < n_fft), frame f at f * hop, no padding, no detrending.
 *   window_dev: n_fft doubles; twiddle_dev: exp(-2 pi i k / n_fft), k < n_fft / 2, interleaved (re, im) doubles.
 *   For bins k = 0 .. n_fft / 2, X_f = FFT(w x'_f), Y_f = FFT(w y'_f) in float64 (one complex transform carries both):
 *     Sxx = sum_f |X_f|^2,  Syy = sum_f |Y_f|^2,  Sxy = sum_f conj(X_f) Y_f.
 * ira_xspec_accumulate: grid (chunk of IRA_XSPEC_FRAMES frames, pair); a workgroup adds the frames of its chunk in
 *   ascending order in registers and writes partial_dev[((p * chunks + c) * 4 + s) * nbins + k], s = Sxx, Syy, Re Sxy,
 *   Im Sxy, nbins = n_fft / 2 + 1, chunks = ceil(max_frames / IRA_XSPEC_FRAMES), with plain stores (no atomics).  Chunks
 *   at or past ceil(K / IRA_XSPEC_FRAMES) of a pair are not written, and nothing past a row's n_dev[p] samples is read.
 *   The chunk size is a constant, so a pair's sums are the same bytes whatever else is in the batch.  A channel whose
 *   windowed frame is all zeros contributes the spectrum 0 exactly (not the other channel's rounding error).
 * ira_xspec_finish: one thread per (pair, bin) adds the pair's chunks in ascending order and writes out_dev[(p *
 *   IRA_XSPEC_ROWS + r) * nbins + k], float64, r = 0 Sxx  1 Syy  2 Re Sxy  3 Im Sxy  4, 5 H1 = Sxy / Sxx (re, im)
 *   6, 7 H2 = Syy / conj(Sxy) = Syy Sxy / |Sxy|^2 (re, im)  8 coherence = min(1, |Sxy|^2 / (Sxx Syy))
 *   9 10 log10 |H1|^2 dB  10 atan2(Im Sxy, Re Sxy) radians.  A quotient whose denominator is 0 is NaN; each operation
 *   rounds once (no contraction).  A pair without frames has zero sums.
 * max_frames >= every pair's K (it sizes the grid and the partial array); npairs <= 65535.  NULL pointers: IRA_E_NULL;
 * n_fft, hop or a count out of range: IRA_E_SIZE; both before anything is launched.  npairs = 0: IRA_OK, no launch. */
#define IRA_XSPEC_FRAMES 16   /* frames per chunk: a constant, never sized from the batch or the device */
#define IRA_XSPEC_ROWS 11
int32_t ira_xspec_accumulate(const float* x_dev, const int64_t* x_off_dev, const int64_t* y_off_dev,
                             const int64_t* n_dev, int32_t npairs, int32_t max_frames, int32_t n_fft, int32_t hop,
                             const double* window_dev, const double* twiddle_dev, double* partial_dev, void* stream);
int32_t ira_xspec_finish(const double* partial_dev, const int64_t* n_dev, int32_t npairs, int32_t max_frames,
                         int32_t n_fft, int32_t hop, double* out_dev, void* stream);

/* ---- Normalized echo density (Abel & Huang): sliding-window fraction of samples outside the window's own sigma ---------
 * Nothing in the reference computes it (its "echo density proxy" is ira_diffusion's count over hard windows against a
 * user threshold); the entry point replaces no reference function.  Host side, with the definition pinned:
 * audio_analysis_amd/analyse/echodensity.py (`python -m analyse.echodensity`).
 * ira_echo_density: channel c is len_dev[c] float32 samples at x_dev + off_dev[c]; o = max(onset_dev[c], 0) is read on the
 *   device.  w_dev: W = 2 delta + 1 float64 weights (> 0), built on the host.  K = 0 if len <= o, else min((len - 1 - o) /
 *   step + 1, kmax); position j < K has its centre at c = o + j step and the window i = c - delta .. c + delta clipped
 *   to [0, len), k = i - (c - delta).  With h2[i] = float64(x[i])^2 and, over the clipped window with k ascending,
 *   A = sum w[k], B = sum w[k] h2[i], C = sum of w[k] where h2[i] A > B (1 + 2^-32):
 *     prof_dev[prof_off_dev[c] + j] = float32((C / A) / 0.31731050786291415), the NaN IRA_NED_NAN_SILENT where B == 0 and
 *     the NaN IRA_NED_NAN_NONFINITE where B is not finite.  Row c must hold the K of onset 0 (min((len - 1) / step + 1,
 *     kmax), 0 for len = 0) floats: the onset never returns to the host to size it; entries from K on are NaN.
 *   rec_dev[c * IRA_NED_DOUBLES + ..], reduced from the float32 row as stored: [0] K  [1] positions with B == 0
 *     [2] positions with B not finite  [3] the maximum of the other values (NaN for none)  [4] its first index (-1)
 *     [5..7] the first j with prof[j] >= thresholds[t], t < nthr (-1 for none and for unused slots); NaN never crosses.
 *   thresholds is a HOST array of nthr doubles (0..IRA_NED_MAX_THRESHOLDS, finite; NULL only with nthr = 0), checked
 *   like delta (1..IRA_NED_MAX_DELTA), step (>= 1), kmax (0..2^31) and nch (0..65535) before anything is launched:
 *   IRA_E_NULL / IRA_E_SIZE.  nch = 0: IRA_OK, no launch.  No scratch.
 *   A workgroup stages float64 squares of IRA_NED_TILE positions' span (fewer for large steps and windows) and the
 *   weights in LDS, one thread per position; a position's sums are a function of its own window in one fixed order, and
 *   there are no atomics: a channel's row and record are bit-identical whatever the batch or the channel's place in it. */
#define IRA_NED_DOUBLES 8
#define IRA_NED_TILE 1024          /* positions a workgroup takes at a time when their span fits (always at step 1) */
#define IRA_NED_MAX_DELTA 2048     /* W <= 4097: 20 ms at 192 kHz is 3841 */
#define IRA_NED_MAX_THRESHOLDS 3
#define IRA_NED_NAN_SILENT 0x7fc00000u
#define IRA_NED_NAN_NONFINITE 0x7fc00001u
int32_t ira_echo_density(const float* x_dev, const int64_t* off_dev, const int64_t* len_dev, const int64_t* onset_dev,
                         int32_t nch, const double* w_dev, int32_t delta, int32_t step, int64_t kmax,
                         const double* thresholds, int32_t nthr, float* prof_dev, const int64_t* prof_off_dev,
                         double* rec_dev, void* stream);

/* ---- Early reflections: the energy-time curve from the onset, its outstanding local maxima, ITDG and DRR sums ----------
 * Nothing in the reference computes it; the entry point replaces no reference function.  Host side, with the definition
 * pinned: audio_analysis_amd/analyse/reflections.py (`python -m analyse.reflections`).
 * ira_reflections: channel c is len_dev[c] float32 samples at x_dev + off_dev[c]; o = max(onset_dev[c], 0) is read on the
 *   device.  w_dev: W = 2 d + 1 float64 weights (> 0), built on the host.  h2[i] = float64(x[i])^2, 0 outside the channel;
 *   e[n] = sum_k w[k] h2[n - d + k] from 0.0 with k ascending, one rounding per multiply and per add.
 *   erow_dev[erow_off_dev[c] + j] = e[o + j], j < R = min(len - o, Rmax), Rmax = D + Tn + B (Tn >= 2^40: no bound).  Row c
 *     must hold the R of onset 0 (min(len, Rmax)) doubles: the onset never returns to the host to size it; entries from R
 *     on are NaN.  max_room is the longest row of the batch; it sizes the grids and the scratch, no value depends on it.
 *   n0 = the first index of the maximum of e over [o, min(len, o + D)) (a NaN never wins), Ed = e[n0].  A candidate is an
 *     n in [n0 + G, min(len, n0 + Tn + 1)) with  e[n] > e[m] for m in [n - S, n);  e[n] >= e[m] for m in (n, min(n + S,
 *     len - 1)];  e[n] >= Ed rel;  e[n] cnt >= prom Bsum, Bsum the sum of e[m] over [max(n - B, n0 + G), n - S) and then
 *     (n + S, min(n + B, len - 1)], added one at a time with m ascending from 0.0, cnt its number of terms (cnt = 0 or
 *     Bsum = 0 passes).  Of the M candidates the min(M, keep) of largest e are kept (the earlier on equal e).
 *   list_dev[(c * keep + i) * IRA_REFL_FIELDS + ..], the kept in ascending time: [0] n  [1] e[n]  [2] Bsum  [3] cnt
 *     [4] m = the first index of max |x| over [max(n - d, 0), min(n + d, len - 1)]  [5] x[m]; unused rows hold -1 in [0],
 *     [3], [4] and NaN in the others.
 *   rec_dev[c * IRA_REFL_DOUBLES + ..]: [0] n0  [1] Ed  [2] M  [3] the number kept  [4] the first candidate in time (-1:
 *     none)  [5] sum of h2 over [max(n0 - Dw, 0), min(n0 + Dw, len - 1)]  [6] sum of h2 over (n0 + Dw, len)  [7] the
 *     non-finite values among the R row entries.  len <= o: n0 = o, Ed = NaN, zeros and -1.
 *   scratch_dev: nch * ceil(max_room / IRA_REFL_TILE) * (1 + 4 * ceil(IRA_REFL_TILE / (S + 1))) doubles (a count and the
 *     candidates of every tile), checked against scratch_doubles.
 *   Checked before anything is launched (IRA_E_NULL / IRA_E_SIZE): d 1..IRA_REFL_MAX_HALF, D 1..IRA_REFL_MAX_DIRECT,
 *   Dw >= 1, 1 <= S <= 1024, G >= S, S < B <= IRA_REFL_MAX_BG, Tn >= 0, rel >= 0 and prom >= 1 finite, keep
 *   1..IRA_REFL_MAX_KEEP, nch 0..65535, max_room 0..Rmax.  nch = 0: IRA_OK, no launch.
 *   Four launches (envelope, direct sound, candidates, selection), no atomics; every sum runs in one fixed order that
 *   depends on the channel alone: a channel's outputs are bit-identical whatever the batch or the channel's place in it. */
#define IRA_REFL_DOUBLES 8
#define IRA_REFL_FIELDS 6
#define IRA_REFL_TILE 1024         /* row entries a workgroup of the envelope and candidate launches takes */
#define IRA_REFL_MAX_HALF 512      /* W <= 1025 */
#define IRA_REFL_MAX_DIRECT 1024
#define IRA_REFL_MAX_BG 2048
#define IRA_REFL_MAX_KEEP 64
int32_t ira_reflections(const float* x_dev, const int64_t* off_dev, const int64_t* len_dev, const int64_t* onset_dev,
                        int32_t nch, const double* w_dev, int32_t d, int32_t D, int32_t Dw, int32_t G, int32_t S,
                        int32_t B, int64_t Tn, double rel, double prom, int32_t keep, int64_t max_room,
                        double* erow_dev, const int64_t* erow_off_dev, double* scratch_dev, int64_t scratch_doubles,
                        double* list_dev, double* rec_dev, void* stream);

/* ---- Frequency-dependent-window (FDW) response: one windowed Fourier sum per frequency point, window of N cycles ----------
 * Nothing in the reference computes it; the entry points replace no reference function.  Host side, with the definition
 * pinned: audio_analysis_amd/analyse/fdw.py (`python -m analyse.fdw`).
 * ira_fdw_response: channel c is len_dev[c] float32 samples at x_dev + off_dev[c]; its centre p = centre_dev[c] (int64) is
 *   read on the device and may lie outside the channel.  Point j < npts has rho[j] = f_j / fs (float64, 0 < rho <= 0.5) and
 *   a half width half[j] = H >= 1 samples, the same for every channel.  Terms k = -H .. H, i = p + k; a term with i outside
 *   [0, len) contributes nothing and is not read.
 *     weight   window 0 (hann): w(k) = 0.5 + 0.5 cospi(k / (H + 1)), formed as sinpi((H + 1 - |k|) / (2 H + 2))^2, the
 *              same function without the cancellation at the window's ends (> 0 on every term, 1 at the centre);
 *              window 1 (rect): w = 1
 *     phasor   t_hi = k * rho, t_lo = fma(k, rho, -t_hi), r = (t_hi - rint(t_hi)) + t_lo (the turn count reduced exactly),
 *              e^{-2 pi i r} from sincospi(2 r)
 *     v = w(k) * float64(x[i]);  S0 = sum v e^{-2 pi i r};  S1 = sum k v e^{-2 pi i r};  A = sum |v|;  N = the number of
 *     terms inside the channel.
 *   out_dev[(c * npts + j) * IRA_FDW_FIELDS + ..], float64: [0] Re S0  [1] Im S0  [2] Re S1  [3] Im S1  [4] A  [5] N.
 *   N = 0 gives zeros.  Non-finite samples propagate by arithmetic alone: a NaN or an infinity inside a point's window
 *   makes that point's sums non-finite and no other point's.
 *   rho and half are HOST arrays, checked before anything is launched; rho_dev and half_dev are the same values on the
 *   device (the kernels read them there: this is the one argument pair more than a host-only table would need, the
 *   library copies nothing itself).  Checked (IRA_E_NULL / IRA_E_SIZE): nch 0..65535, npts 0..IRA_FDW_MAX_POINTS, every
 *   half 1..IRA_FDW_MAX_HALF, every rho finite and in (0, 0.5], window 0 or 1, scratch_doubles >=
 *   ira_fdw_scratch_doubles(nch, half, npts).  nch = 0 or npts = 0: IRA_OK, no launch.
 *   A point with H <= IRA_FDW_NARROW_HALF (at most 255 terms) is NARROW: one wavefront takes it, four points per
 *   workgroup, lane l adds the terms l, l + 64, .. in ascending order and the lanes are added by a butterfly.  Any other
 *   point is WIDE: it is cut into ceil((2 H + 1) / IRA_FDW_CHUNK) chunks of IRA_FDW_CHUNK consecutive terms, a workgroup
 *   of 256 threads takes one (chunk, channel), thread t adds the terms t, t + 256, .. of the chunk in ascending order,
 *   lanes by a butterfly, the four waves in ascending order; the chunk's five sums go to scratch with plain stores and a
 *   finishing launch adds a point's chunks in ascending order.  The job tables (chunk -> point, first chunk of a point,
 *   the narrow points) are built on the device from half_dev by a one-workgroup launch into the tail of scratch.
 *   Four launches, no atomics; the sums of a (channel, point) are a function of that channel's samples, p, rho, H and
 *   the window alone and run in one fixed order: bit-identical whatever the batch or the channel's place in it.
 * ira_fdw_scratch_doubles: nch * T * IRA_FDW_SUMS + (npts + 1 + T + M + 1) / 2 doubles, T the chunks of the wide points and M
 *   the number of narrow points (the second term holds the int32 tables); IRA_E_NULL / IRA_E_SIZE (negative) as above. */
#define IRA_FDW_FIELDS 6
#define IRA_FDW_SUMS 5             /* Re S0, Im S0, Re S1, Im S1, A of a chunk; N needs no sum */
#define IRA_FDW_MAX_POINTS 4096
#define IRA_FDW_MAX_HALF (1 << 20)
#define IRA_FDW_CHUNK 4096         /* terms per partial sum: a constant, never sized from the batch or the device */
#define IRA_FDW_NARROW_HALF 127    /* 2 H + 1 <= 255 terms: one wavefront per point */
int64_t ira_fdw_scratch_doubles(int32_t nch, const int32_t* half, int32_t npts);
int32_t ira_fdw_response(const float* x_dev, const int64_t* off_dev, const int64_t* len_dev, const int64_t* centre_dev,
                         int32_t nch, const double* rho, const int32_t* half, const double* rho_dev,
                         const int32_t* half_dev, int32_t npts, int32_t window, double* scratch_dev,
                         int64_t scratch_doubles, double* out_dev, void* stream);

/* ---- Burst decay: a constant-Q level-over-periods map, one windowed Fourier sum per (channel, point, step) -----------------
 * Nothing in the reference computes it; the entry points replace no reference function.  Host side, with the definition
 * pinned: audio_analysis_amd/analyse/burstdecay.py (`python -m analyse.burstdecay`).
 * Point j < npts has rho[j] = f_j / fs (float64, 0 < rho <= 0.5) and a half width half[j] = H >= 1 samples, as for
 * ira_fdw_response.  Its WAVELET is g_j(k) = w(k) e^{-2 pi i r(k)}, k = -H .. H, with w and r formed exactly as stated there:
 *     weight   window 0 (hann): w(k) = sinpi((H + 1 - |k|) / (2 H + 2))^2;  window 1 (rect): w = 1
 *     phasor   t_hi = k * rho, t_lo = fma(k, rho, -t_hi), r = (t_hi - rint(t_hi)) + t_lo, (sn, cs) from sincospi(2 r)
 *     g_j(k) = (w * cs, -(w * sn))
 * ira_burst_table: writes g_j(k) as (re, im) doubles at table_dev[2 * (tab_off[j] + k + H)], tab_off[j] (int64, read from
 *   tab_off_dev) the first entry of point j.  Every entry is a function of (rho_j, H_j, window, k) alone; one thread per
 *   entry, one launch.  rho and half are HOST arrays, checked before anything is launched, rho_dev and half_dev the same
 *   values on the device (the library copies nothing itself).  Checked (IRA_E_NULL / IRA_E_SIZE): npts
 *   0..IRA_FDW_MAX_POINTS, every half 1..IRA_FDW_MAX_HALF, every rho finite and in (0, 0.5], window 0 or 1, table_doubles
 *   >= ira_burst_table_doubles(half, npts).  A point whose entries tab_off[j] .. tab_off[j] + 2 H would leave the
 *   table_doubles / 2 entries is not written.  npts = 0: IRA_OK, no launch.
 * ira_burst_decay: channel c is len_dev[c] float32 samples at x_dev + off_dev[c]; its centre p = centre_dev[c] (int64) is
 *   read on the device and may lie outside the channel.  Step m < nsteps of point j is centred on c = p + delta[j * nsteps
 *   + m] (int32):
 *     S[j, m] = sum over k = -H .. H of g_j(k) * float64(x[c + k]);  a term with c + k outside [0, len) contributes nothing
 *     and is not read.  The phase is relative to the cell's own centre.
 *   out_dev[((c * npts + j) * nsteps + m) * 2 + {0, 1}] = Re S, Im S, float64.  A cell with nothing inside is (0, 0).
 *   Non-finite samples propagate by arithmetic alone: a NaN or an infinity inside a cell's window makes that cell
 *   non-finite and no other.
 *   ONE ORDER, of a cell's terms u = k + H = 0 .. 2 H: lane l < IRA_BURST_LANES adds the terms u = l, l + 64, l + 128, ..
 *   in ascending order from (0, 0) by re = fma(Re g, x, re), im = fma(Im g, x, im); the 64 lane sums are then added in
 *   ascending lane order, starting from lane 0's.  A term outside the channel is skipped or enters as x = +0.0, which are
 *   the same bits (no sum here can be -0.0).  The order depends on H and k alone: a cell's bits are a function of the
 *   channel's samples, p, delta[j, m], H, rho and the window only -- identical whatever the batch, the channel's place
 *   or alignment in it, and whichever other points and steps the call carries.
 *   Tiling (no value depends on it): one wavefront takes IRA_BURST_STEPS consecutive steps of one (channel, point) and
 *   walks the window once, a ROUND of IRA_BURST_LANES consecutive terms at a time: g_j of the round is loaded once (16
 *   bytes a lane) and serves every step of the tile, whose samples are IRA_BURST_STEPS loads of 64 consecutive floats.
 *   Rounds in which every step of the tile lies inside its channel run without a test; the others compare u with each
 *   step's first and last term inside.  The lane sums meet in LDS (pitch IRA_BURST_LANES + 1 doubles).  A workgroup is
 *   IRA_BURST_CHANNELS waves: consecutive channels of the same (point, step tile), which walk the same wavelet at the
 *   same time; the workgroups are numbered so that one XCD takes consecutive tiles and points of the same channels,
 *   whose samples overlap, and finds them in its L2.  One launch, no atomics, no scratch.
 *   half and delta are HOST arrays, checked before anything is launched; half_dev, delta_dev the same values on the
 *   device.  Checked (IRA_E_NULL / IRA_E_SIZE): nch 0..65535, npts 0..IRA_FDW_MAX_POINTS, nsteps 0..IRA_BURST_MAX_STEPS,
 *   every half 1..IRA_FDW_MAX_HALF, |delta| <= IRA_BURST_MAX_DELTA and delta non-decreasing in m for every j,
 *   table_doubles >= ira_burst_table_doubles(half, npts).  The device's own copies are clamped to the same ranges and a
 *   point whose tab_off would leave the table gives NaN cells, so no access leaves x's channels, table_dev or out_dev
 *   even if the device arrays do not hold the host's values.  nch, npts or nsteps = 0: IRA_OK, no launch.
 * ira_burst_table_doubles (host only): 2 * sum over j of (2 half[j] + 1), the doubles of the wavelet table -- the only
 *   workspace the two calls share; IRA_E_NULL / IRA_E_SIZE (negative) as above. */
#define IRA_BURST_STEPS 8          /* steps of a point a wavefront serves from one walk over the wavelet */
#define IRA_BURST_LANES 64         /* terms per round, one a lane: constants, never sized from the batch or the device */
#define IRA_BURST_CHANNELS 4       /* waves, i.e. channels, per workgroup */
#define IRA_BURST_MAX_STEPS 4096
#define IRA_BURST_MAX_DELTA (1 << 24)
int64_t ira_burst_table_doubles(const int32_t* half, int32_t npts);
int32_t ira_burst_table(const double* rho, const int32_t* half, const double* rho_dev, const int32_t* half_dev,
                        const int64_t* tab_off_dev, int32_t npts, int32_t window, double* table_dev, int64_t table_doubles,
                        void* stream);
int32_t ira_burst_decay(const float* x_dev, const int64_t* off_dev, const int64_t* len_dev, const int64_t* centre_dev,
                        int32_t nch, const int32_t* half, const int32_t* half_dev, const int64_t* tab_off_dev,
                        const double* table_dev, int64_t table_doubles, const int32_t* delta, const int32_t* delta_dev,
                        int32_t npts, int32_t nsteps, double* out_dev, void* stream);

/* ---- Minimum phase, excess phase and the minimum-phase response by the real cepstrum ---------------------------------------
 * Nothing in the reference computes it; the entry points replace no reference function.  Host side, with the definition
 * pinned: audio_analysis_amd/analyse/minphase.py (`python -m analyse.minphase`).
 * The chain of a channel x of D samples with the centre p, N a power of two (32 .. 2^IRA_MINPHASE_MAX_LOG2):
 *     X         = rfft(x[:D], n = N)                                    (ira_rfft_smooth / ira_rfft_any, data_len D, win_len N)
 *     P         = max_k |X_k|^2, |X|^2 = re * re + im * im in float64;  P_floor = P * 10^(floor_db / 10)
 *     G_k       = 0.5 ln(max(|X_k|^2, P_floor)), k = 0 .. N/2, written as the complex (G, 0)          (ira_minphase_logmag)
 *     c         = float32(irfft(G, N))                                  (ira_band_irfft*, all-pass record 2, -1, -1)
 *     T         = rfft(c[0 : N/2], n = N)                               (data_len N/2)
 *     phi_min_k = 2 Im T_k: the folded cepstrum c[0], 2 c[n], c[N/2], 0 .. has exactly this imaginary transform
 *     phi_rel_k = atan2(Im X_k, Re X_k) + 2 pi ((k p mod N) / N), k p mod N in int64
 *     d_k       = phi_rel_k - phi_min_k;  wrapped: d_k - 2 pi rint(d_k / (2 pi))                      (ira_minphase_excess)
 *     excess    = numpy.unwrap of the wrapped d over k = 0 .. N/2                                     (ira_phase_unwrap)
 *     M_k       = e^{G_k} (cos phi_min_k, sin phi_min_k), Im M = 0 at k = 0 and N/2, in place of G    (ira_minphase_spectrum)
 * Element e < nb: nfft_dev[e] = N (int32) and its N/2 + 1 bins at spec_off_dev[e] (int64), counted in complex doubles for
 * spec_dev, tspec_dev and g_dev and in doubles for excess_dev / unwrapped_dev -- the offsets ira_phase_unwrap takes.
 * ira_minphase_logmag: pmax_dev[e] = P as the maximum over the bit patterns of |X_k|^2 (sign cleared), so a NaN among them
 *   wins; floored_dev[e] (int64) = the bins with |X_k|^2 < P_floor.  Both are zeroed by the call and combined across
 *   workgroups by INTEGER atomics (max, add): order free.  An element has values only if 0 < P < infinity; otherwise (digital
 *   silence, a NaN or an infinity among the samples) its G is (0, 0) -- no logarithm of zero is taken -- its floored count 0,
 *   and the other calls write 0 (excess, M) or NaN (the records) for it.  Elements never meet: no value of one element
 *   depends on another.
 * ira_minphase_gather: out_dev[(e * npts + j) * IRA_MINPHASE_FIELDS + ..], float64, for the bin k = bins_dev[e * npts + j]
 *   (int32, clamped to 1 .. N/2 - 1):  [0] Re X_k  [1] Im X_k  [2] Im T_(k-1)  [3] Im T_k  [4] Im T_(k+1)
 *   [5] excess_(k-1)  [6] excess_k  [7] excess_(k+1)  (radians, unwrapped).
 * All four are streaming passes (16-byte loads of the interleaved complex doubles, one bin a lane); no value depends on the
 * launch shape, and every index is formed from the element's own clamped N.
 * Checked before anything touches a device (IRA_E_NULL / IRA_E_SIZE): nb 0..65535, max_nfft (the largest N; it sizes the
 * grid) a power of two 32 .. 2^IRA_MINPHASE_MAX_LOG2, IRA_MINPHASE_MIN_FLOOR_DB <= floor_db <= 0, npts
 * 0..IRA_FDW_MAX_POINTS.  nb = 0 (or npts = 0): IRA_OK, no launch. */
#define IRA_MINPHASE_FIELDS 8
#define IRA_MINPHASE_MAX_LOG2 21          /* the largest transform the long-FFT kernels take */
#define IRA_MINPHASE_MIN_FLOOR_DB (-300.0)
int32_t ira_minphase_logmag(const double* spec_dev, const int64_t* spec_off_dev, const int32_t* nfft_dev, int32_t nb,
                            int32_t max_nfft, double floor_db, double* g_dev, double* pmax_dev, int64_t* floored_dev,
                            void* stream);
int32_t ira_minphase_excess(const double* spec_dev, const double* tspec_dev, const int64_t* spec_off_dev,
                            const int32_t* nfft_dev, const int64_t* centre_dev, const double* pmax_dev, int32_t nb,
                            int32_t max_nfft, double* excess_dev, void* stream);
int32_t ira_minphase_gather(const double* spec_dev, const double* tspec_dev, const double* unwrapped_dev,
                            const int64_t* spec_off_dev, const int32_t* nfft_dev, const int32_t* bins_dev,
                            const double* pmax_dev, int32_t nb, int32_t npts, double* out_dev, void* stream);
int32_t ira_minphase_spectrum(double* g_dev, const double* tspec_dev, const int64_t* spec_off_dev, const int32_t* nfft_dev,
                              const double* pmax_dev, int32_t nb, int32_t max_nfft, void* stream);

/* ---- MLS impulse-response measurement: circular correlation with a maximum-length sequence by the fast Hadamard transform ---
 * Nothing in the reference computes it; the entry points replace no reference function.  Host side, with the definition
 * pinned: audio_analysis_amd/analyse/mls.py (`python -m analyse.mls`); the tables are made by engine_geometry.mls_tables.
 * One order m per call (IRA_MLS_MIN_ORDER .. IRA_MLS_MAX_ORDER), P = 2^m - 1, R = periods (1 .. IRA_MLS_MAX_PERIODS, one
 * value per call).  Channel e < nb reads the R P samples x_dev[begin_dev[e] ..] (int64 offsets into x_dev) and owns row e of
 * the workspace w_dev, 2^m doubles at w_dev + e 2^m:
 *     Y[n]  = sum over r = 0 .. R-1, ascending from 0.0, of (double) x[b + r P + n],  n < P
 *     w     = zeros(2^m);  w[G[n]] = Y[n]            (g_dev: int32 (P,), a permutation of 1 .. P)              (ira_mls_fold)
 *     E     = sum Y[n]^2;  D = sum over n and r of ((double) x[b + r P + n] - Y[n] / R)^2, 0 when R = 1         (ira_mls_fold)
 *     W     = the Walsh-Hadamard transform of w in natural order: stages h = 1, 2, 4 .. 2^(m-1) in that order, each
 *             (lo, hi) -> (lo + hi, lo - hi) with lo the lower index                                        (ira_mls_hadamard)
 *     h[k]  = float32((W[out[k]] - W[0]) / (double)(2^m R)),  k < P   (out_dev: int32 (P,), a permutation of 1 .. P), written
 *             at h_dev[h_off_dev[e] + k]; nothing else of h_dev is touched                                    (ira_mls_finish)
 * W[0] is sum Y, so h is the circular correlation with the +-1 sequence with its DC value restored; the stage order fixes
 * every rounding, so W equals a NumPy restatement of the same stages bit for bit.
 * ira_mls_fold: sums_dev[2 e] = E, sums_dev[2 e + 1] = D.  Thread t of workgroup j of a channel (IRA_MLS_FOLD_THREADS
 *   threads; B = min(ceil(P / IRA_MLS_FOLD_THREADS), IRA_MLS_FOLD_BLOCKS) workgroups) takes n = (j + i B)
 *   IRA_MLS_FOLD_THREADS + t, i ascending, and adds Y^2 -- and, r ascending within n, the residual squares -- to its own
 *   sums; a workgroup adds its threads' sums in a fixed tree (xor butterfly over 64 lanes, then the 4 waves ascending) and
 *   writes the pair to scratch_dev; a second launch adds a channel's B pairs ascending from 0.0.  No float atomics: the sums
 *   are the same in every call and batch.  scratch_dev: 2 nb B doubles; engine_geometry.mls_scratch_bytes(nb, m) =
 *   8 nb (2^m + 2 B) is the workspace and the scratch together.
 * ira_mls_hadamard: tiles of 2^IRA_MLS_TILE_LOG2 doubles in LDS, 16 elements a thread in registers.  m <= 12: one pass;
 *   13 .. 20: a second over the bits 12 .. m-1; 21: 12 + 5 + 4 bits (engine_geometry.mls_pass_plan).
 * Table values are masked to m bits before they index a row.  Checked before anything touches a device (IRA_E_NULL /
 * IRA_E_SIZE): NULL pointers, nb 0..65535, the order, the periods.  nb = 0: IRA_OK, no launch.  Vector stores only. */
#define IRA_MLS_MIN_ORDER 2
#define IRA_MLS_MAX_ORDER 21
#define IRA_MLS_MAX_PERIODS 1024
#define IRA_MLS_TILE_LOG2 12              /* the tile order T of ira_mls_hadamard: 2^12 doubles = 32 KiB of LDS */
#define IRA_MLS_FOLD_THREADS 256
#define IRA_MLS_FOLD_BLOCKS 128           /* the most workgroups of ira_mls_fold (and ira_mls_finish) along a channel */
int32_t ira_mls_fold(const float* x_dev, const int64_t* begin_dev, int32_t nb, int32_t order, int32_t periods,
                     const int32_t* g_dev, double* w_dev, double* sums_dev, double* scratch_dev, void* stream);
int32_t ira_mls_hadamard(double* w_dev, int32_t nb, int32_t order, void* stream);
int32_t ira_mls_finish(const double* w_dev, const int32_t* out_dev, int32_t nb, int32_t order, int32_t periods, float* h_dev,
                       const int64_t* h_off_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IRA_H_ */
