// Launchers of the specialised STFT kernels.  The extern "C" entry points in ira_stft.hip are the only code that decides
// which kernel serves which (precision, n_fft, layout); a launcher sizes and launches its kernel for the configuration it
// is given and tests nothing else.
#pragma once
#include "ira_common.h"

// stft3_kernel (ira_stft3.hip): float32 / n_fft 4096, (F, T) layout
int32_t ira_stft3_launch(const float* x, const int64_t* off, const int32_t* nframes, int32_t nseg, int32_t max_frames,
                         int32_t hop, const void* window, const void* tw, double floor_db, float* out,
                         const int64_t* out_off, const int32_t* frame_sel, const int64_t* sel_off, hipStream_t st);

// stft6_kernel (ira_stft3.hip): float32 / n_fft 4096, frame-major (T, F) layout.  tail != nullptr (and no frame selection):
// the suffix energies of ira_tail_energy for these segments; a frame whose suffix is under the floor stores the floor
// without loading or transforming anything.  Same bytes either way.
int32_t ira_stft6_launch(const float* x, const int64_t* off, const int32_t* nframes, int32_t nseg, int32_t max_frames,
                         int32_t hop, const void* window, const void* tw, double floor_db, float* out,
                         const int64_t* out_off, const int32_t* frame_sel, const int64_t* sel_off, const double* tail,
                         const int64_t* tail_off, hipStream_t st);

// stft2_kernel (ira_stft2.hip): float32 / 8192, float64 / 4096 and float64 / 8192, (F, T) layout
int32_t ira_stft2_launch(const float* x, const int64_t* off, const int32_t* nframes, int32_t nseg, int32_t max_frames,
                         int32_t n_fft, int32_t hop, const void* window, const void* tw, int32_t precision,
                         double floor_db, float* out, const int64_t* out_off, const int32_t* frame_sel,
                         const int64_t* sel_off, hipStream_t st);

// stft5_kernel (ira_stft4.hip): float64 / n_fft 8192, a grid of ceil(max_frames / 8) x nseg workgroups of eight consecutive
// frames.  lb_nbins <= 0: the frame-major (T, F) dB matrix; lb_nbins > 0: the (lb_nbins, T) log-bin curves of ira_stft_logbin.
// tail != nullptr (and no frame selection): the suffix energies of ira_tail_energy (ira_tailenergy.hip) for these segments;
// stft5_consts_kernel (one workgroup, ahead of the launch) then fills `consts` with the window's greatest square and the
// floored log-bin row, and a workgroup whose suffix is under the floor stores that row and leaves.  Same bytes either way.
int32_t ira_stft5_launch(const float* x, const int64_t* off, const int32_t* nframes, int32_t nseg, int32_t max_frames,
                         int32_t hop, const void* window, const void* tw, double floor_db, float* out,
                         const int64_t* out_off, const int32_t* frame_sel, const int64_t* sel_off, int32_t lb_nbins,
                         int32_t lb_kbase, const int32_t* lb_first, const int32_t* lb_count, const double* tail,
                         const int64_t* tail_off, void* consts, hipStream_t st);
