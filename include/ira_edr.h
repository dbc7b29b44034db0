/* libira: energy decay relief (Jot's EDR: the Schroeder backward integration at every frequency of a short-time transform).
 * A third header beside ira.h and ira_equalise.h: the entry points below belong to the same library (libira.so,
 * IRA_ABI_VERSION of ira.h, unchanged) and follow its conventions -- extern "C", device pointers + sizes, hipStream_t as
 * void*, an int32 status (IRA_OK, IRA_E_NULL, IRA_E_SIZE, ...).  audio_analysis_amd/_lib.py binds them from EDR_PROTOTYPES
 * after the tables of ira.h and ira_equalise.h. */
#ifndef IRA_EDR_H
#define IRA_EDR_H

#include "ira.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Energy decay relief: band powers of the frames, their backward sums along the frame axis, the dB curves -------------------
 * Nothing in the reference computes it; the entry points replace no reference function.  Host side, with the definition
 * pinned: audio_analysis_amd/analyse/edr.py (`python -m analyse.edr`).
 * Segment s: n_dev[s] float32 samples at x_dev + x_off_dev[s].  n_fft a power of two 256 .. 8192, 1 <= hop <= n_fft,
 *     T = 1 + (n - n_fft) / hop frames (0 when n < n_fft), frame m at m * hop, no padding; window_dev n_fft doubles,
 *     twiddle_dev the n_fft / 2 complex doubles exp(-2 pi i k / n_fft).
 * Row j < nrows: the rFFT bins [first_j, first_j + count_j) within 0 .. n_fft / 2 (int32 tables; first is masked into
 *     0 .. n_fft / 2 + 1 and count into what is left of the bins before they index anything).  count_j = 0 is a legal,
 *     empty row: its powers are 0.0.
 *     P(m, j) = sum over the row's bins k of re * re + im * im of X_m[k], X_m the transform of the windowed frame, float64.
 * The order of a row's sum depends on (n_fft, first_j, count_j) alone:
 *     count <= IRA_EDR_SERIAL: from 0.0, the bins in ascending order;
 *     else: 32 partial sums, partial l from 0.0 over the bins first + l, first + l + 32, ... ascending, then five rounds of
 *     v[l] = v[l] + v[l ^ d], d = 16, 8, 4, 2, 1.
 * Layout of P (ira_edr_power writes it, ira_edr_integrate reads it): p_dev[p_off_dev[s] + j * Tpad_s + m],
 *     Tpad_s = ceil(T_s / IRA_EDR_FRAMES) * IRA_EDR_FRAMES; the columns T_s .. Tpad_s - 1 hold 0.0
 *     (audio_analysis_amd.engine_geometry.edr_layout restates it).
 * ira_edr_power: grid (chunk of IRA_EDR_FRAMES frames, segment); a workgroup walks its chunk two frames at a time, frames m
 *     and m + 1 as the real and the imaginary part of ONE complex float64 transform in LDS (a last unpaired frame rides with
 *     zeros), unpacked by conjugate symmetry.  A frame whose windowed samples are all zero has P = 0 exactly; a frame that
 *     holds a non-finite windowed sample has the power NaN in every bin (so NaN in every row that is not empty) and leaves
 *     its partner's spectrum alone.  The bin powers of the pair pass through LDS in bin order, the row sums are staged, and
 *     the chunk's (row, IRA_EDR_FRAMES) block leaves as runs of IRA_EDR_FRAMES doubles (128 bytes) with plain stores (at
 *     n_fft 8192 with more than 254 rows the LDS holds half a chunk's sums: two runs of 64 bytes).  A chunk at or past
 *     Tpad_s / IRA_EDR_FRAMES of a
 *     segment touches no memory; nothing past a segment's last frame is read; a workgroup reads and writes nothing of
 *     another segment.  max_frames >= every segment's T (it sizes the grid).
 * ira_edr_integrate: one wavefront per (segment, row).  With T = T_dev[s] and q = q_dev[s] noise frames (masked into 0 .. T):
 *   The backward sum of a sequence a(0 .. T-1): the frames are cut into blocks of IRA_EDR_BLOCK = 64 counted from the END;
 *     block b holds the frames T - 64 (b + 1) + l, l = 0 .. 63, and 0.0 where that index is negative; six simultaneous steps
 *     d = 1, 2, 4, 8, 16, 32: v[l] = v[l] + v[l + d] for l + d < 64; out[l] = v[l] + carry, carry = 0.0 for block 0 and the
 *     out[0] of block b - 1 after it.
 *     S_raw = the backward sum of P(., j);  N_j = q >= 1 ? S_raw(T - q) / (double)q : 0.0;
 *     S = q >= 1 ? the backward sum of P(m, j) - N_j : S_raw (no subtraction is performed).
 *     L(m, j) = float32(max(10 log10(max(S(m), eps) / S(0)), floor_db)), through the table logarithm of the Schroeder kernels;
 *     S(0) finite and <= eps: every L is floor_db; S(0) NaN: every L is NaN (the maxima keep a NaN, like numpy.maximum).
 *     record (IRA_EDR_DOUBLES doubles at rec_dev + (s * nrows + j) * IRA_EDR_DOUBLES): [0] S(0)  [1] N_j  [2] max over m of
 *     P(m, j)  [3] the first frame of that maximum (numpy.max / numpy.argmax: a NaN wins, the first of them).
 *   curve_dev[c_off_dev[s] + j * T + m] = L(m, j), float32, unpadded (nrows curves of T values: what ira_curve_fits takes);
 *   s_out_dev, optional (NULL: not written): S in the layout of P, padding columns 0.0.
 *   T_dev int32 per segment; a segment with T = 0 writes its record (0, 0, NaN, -1) and nothing else.
 * Both use vector stores only and no atomics; no value depends on the launch shape or on the rest of the batch.
 * Checked before anything touches a device (IRA_E_NULL / IRA_E_SIZE): nseg 0..65535, nrows 1..IRA_EDR_MAX_ROWS, n_fft, hop,
 * max_frames >= 0, eps a finite number >= 0, floor_db finite.  nseg = 0 (or max_frames = 0): IRA_OK, no launch. */
#define IRA_EDR_FRAMES 16     /* frames per chunk and per store run: a constant, never sized from the batch or the device */
#define IRA_EDR_BLOCK 64      /* frames per block of the backward sum */
#define IRA_EDR_MAX_ROWS 256
#define IRA_EDR_SERIAL 16     /* rows of up to this many bins are summed by one thread */
#define IRA_EDR_DOUBLES 4
int32_t ira_edr_power(const float* x_dev, const int64_t* x_off_dev, const int64_t* n_dev, const int64_t* p_off_dev,
                      int32_t nseg, int32_t max_frames, int32_t n_fft, int32_t hop, const double* window_dev,
                      const double* twiddle_dev, const int32_t* row_first_dev, const int32_t* row_count_dev, int32_t nrows,
                      double* p_dev, void* stream);
int32_t ira_edr_integrate(const double* p_dev, const int64_t* p_off_dev, const int32_t* T_dev, const int32_t* q_dev,
                          const int64_t* c_off_dev, int32_t nseg, int32_t nrows, double eps, double floor_db,
                          float* curve_dev, double* rec_dev, double* s_out_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IRA_EDR_H */
