/* libira: equalisation filter design (regularised inverse, minimum-phase FIR).  A second header beside ira.h: the entry
 * points below belong to the same library (libira.so, IRA_ABI_VERSION of ira.h, unchanged) and follow its conventions --
 * extern "C", device pointers + sizes, hipStream_t as void*, an int32 status (IRA_OK, IRA_E_NULL, IRA_E_SIZE, ...).
 * audio_analysis_amd/_lib.py binds them from EQUALISE_PROTOTYPES after the table of ira.h. */
#ifndef IRA_EQUALISE_H
#define IRA_EQUALISE_H

#include "ira.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Equalisation: fractional-octave smoothing on every bin, Kirkeby-Nelson inversion, taper -------------------------------
 * Nothing in the reference computes it; the entry points replace no reference function.  Host side, with the definition
 * pinned: audio_analysis_amd/analyse/equalise.py (`python -m analyse.equalise`).
 * One transform size N per call (nfft, a power of two 32 .. 2^IRA_MINPHASE_MAX_LOG2), n0 = N/2 + 1 bins.  A ROW is one filter:
 *     P_k  = (sum over the row's members m, ascending from 0.0, of (re * re + im * im of X^m_k)) / (double)count  (ira_eq_power)
 *     A_k  = P_k * (Fre * Fre + Fim * Fim), F the row's second spectrum                           (ira_eq_power, spec2_dev given)
 *     pyramid: level 0 = P (or A); level j + 1 has ceil(n_j / 2) entries, L_(j+1)[i] = L_j[2 i] + L_j[2 i + 1], an entry
 *              without a partner is copied; the last level has one entry                                      (ira_eq_pyramid)
 *     W(lo, hi): l = lo, r = hi + 1, left = right = 0.0, j = 0; while l < r: if l is odd left += L_j[l++]; if r is odd
 *              right += L_j[--r]; l >>= 1, r >>= 1, j++.  W = left + right
 *     S_k  = W(lo_k, hi_k) / (double)(hi_k - lo_k + 1)                                                        (ira_eq_smooth)
 *     s = S_k / ref, a = sqrt(s), c_k = (a * t_k + beta_k) / (s + beta_k), then max_gain where c_k > max_gain, written as the
 *              complex (c, 0); the count of bins with c_k > max_gain per row                                  (ira_eq_invert)
 *     f[n] = float32((double)g[n] * v[n]), n < taps                                                           (ira_eq_taper)
 * Every term of a window sum is non-negative and the order of the additions is fixed by (lo, hi) alone: the NumPy restatement
 * (tests/equalise_ref.py) gives the same bits.  The file is built with -ffp-contract=off.
 * Layout of a row's pyramid, N + log2(N) doubles at pyr_dev + row * (N + log2(N)): level j at the offset n_0 + .. + n_(j-1),
 *     n_0 = N/2 + 1, n_(j+1) = (n_j + 1) >> 1, until n_j = 1: log2(N) + 1 levels
 *     (audio_analysis_amd.engine_geometry.equalise_layout restates it; eq_level in ira_equalise.hip serves host and device).
 * ira_eq_power: spectrum i < nspec has its n0 bins at spec_off_dev[i] (int64, counted in complex doubles); row r < nrows takes
 *   the members member_dev[row_first_dev[r] .. row_first_dev[r + 1]) (int32 tables of nmember and nrows + 1 entries; a first
 *   entry is masked into 0 .. nmember, a count into 0 .. IRA_EQ_MAX_MEMBERS and what is left of the table, a member into
 *   0 .. nspec - 1; a row without members gets P = 0).  spec2_dev NULL: P; else the row's F at spec2_off_dev[r].
 * ira_eq_pyramid: the upper levels from level 0, IRA_EQ_TILE_LOG2 levels a pass: a workgroup stages IRA_EQ_TILE entries of the
 *   pass's base level in LDS and writes its share of every level above; ceil(log2(N) / IRA_EQ_TILE_LOG2) passes.
 * ira_eq_smooth: lo_dev, hi_dev int32, n0 entries each, one pair per call; a lane takes one bin; lo is masked into
 *   0 .. N/2 and hi into lo .. N/2 before they index anything.  s_dev: n0 doubles a row, row r at r * n0.
 * ira_eq_invert: ref_dev one double per row; target_dev (t) and beta_dev n0 doubles each, one pair per call; the complex c
 *   of row r goes to c_dev + 2 * c_off_dev[r] (int64, counted in complex doubles).  A row whose ref is not a positive
 *   finite number gets c = 1 and the count 0: no logarithm of zero follows.  clamped_dev (int64 per row) is zeroed by the
 *   call and combined across workgroups by INTEGER atomics.
 * ira_eq_gather: out_dev[r * npts + j] = src_dev[src_off_dev[r] + stride * bins_dev[j]], offsets and stride counted in
 *   doubles (stride 1 for S, 2 for the real parts of c), bins_dev int32 (npts, one table per call) masked into 0 .. N/2.
 * ira_eq_taper: g of row r at g_dev + g_off_dev[r] (float32, at least taps samples), taper_dev taps doubles, f_dev taps
 *   floats a row, row r at r * taps.
 * All six use vector stores only and no floating-point atomics; no value depends on the launch shape, and every index is
 * formed from the call's own N.
 * Checked before anything touches a device (IRA_E_NULL / IRA_E_SIZE): nrows 0..65535, nfft a power of two
 * 32 .. 2^IRA_MINPHASE_MAX_LOG2, nspec and nmember 1 .. 2^24, max_gain a positive finite number, stride 1..2, npts
 * 0..IRA_FDW_MAX_POINTS, 1 <= taps <= nfft / 2.  nrows = 0 (or npts = 0): IRA_OK, no launch. */
#define IRA_EQ_TILE_LOG2 11
#define IRA_EQ_TILE (1 << IRA_EQ_TILE_LOG2)
#define IRA_EQ_MAX_MEMBERS 256
#define IRA_EQ_MAX_TABLE (1 << 24)
int32_t ira_eq_power(const double* spec_dev, const int64_t* spec_off_dev, int32_t nspec, const int32_t* member_dev,
                     int32_t nmember, const int32_t* row_first_dev, int32_t nrows, const double* spec2_dev,
                     const int64_t* spec2_off_dev, int32_t nfft, double* pyr_dev, void* stream);
int32_t ira_eq_pyramid(double* pyr_dev, int32_t nrows, int32_t nfft, void* stream);
int32_t ira_eq_smooth(const double* pyr_dev, const int32_t* lo_dev, const int32_t* hi_dev, int32_t nrows, int32_t nfft,
                      double* s_dev, void* stream);
int32_t ira_eq_invert(const double* s_dev, const double* ref_dev, const double* target_dev, const double* beta_dev,
                      double max_gain, const int64_t* c_off_dev, int32_t nrows, int32_t nfft, double* c_dev,
                      int64_t* clamped_dev, void* stream);
int32_t ira_eq_gather(const double* src_dev, const int64_t* src_off_dev, int32_t stride, const int32_t* bins_dev,
                      int32_t nrows, int32_t npts, int32_t nfft, double* out_dev, void* stream);
int32_t ira_eq_taper(const float* g_dev, const int64_t* g_off_dev, const double* taper_dev, int32_t nrows, int32_t taps,
                     int32_t nfft, float* f_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IRA_EQUALISE_H */
