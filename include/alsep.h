/* alsep.h -- C ABI of libalsep.so, the MI355X (gfx950) kernels behind AudioLab's
 * Process->Separate path.
 *
 * The reference (d8ahazard/AudioLab) is pure Python; it has no FFI for this path.  Each
 * entry point below replaces the arithmetic the reference reaches through the calls cited
 * next to it (paths relative to the reference root).  Binding shown in INTEGRATION.md.
 *
 * Conventions
 *   - Every data pointer is a DEVICE pointer owned by the caller (PyTorch allocator,
 *     tensor.data_ptr()).  The library never frees caller memory.  Objects it creates
 *     (ctx, plan, net) own their private device tables and free them in *_destroy.
 *   - All work is enqueued on the hipStream_t given to alsep_create; calls return after
 *     enqueueing (the caller synchronises).  One ctx per (GPU, stream); not thread-safe.
 *   - Return value: 0 = ok, negative = error; alsep_last_error(ctx) describes the most
 *     recent failure.  No C++ exception crosses the ABI.
 *   - dtype: ALSEP_F32 = float32 storage + f32 MFMA (parity mode),
 *            ALSEP_BF16 = bfloat16 storage + bf16 MFMA with f32 accumulation,
 *            ALSEP_F16  = IEEE half storage + f16 MFMA with f32 accumulation (the type of the reference's
 *                         use_autocast=True, stem_separator.py:106; 8x finer rounding than bf16, range 65504).
 *   - layout of a spectrogram: ALSEP_LAYOUT_REF  = [B,4,dim_f,T]  (the reference's
 *     model I/O, mdxnet.py:56,170; patch_separate.py:52), channels (L_re,L_im,R_re,R_im);
 *     ALSEP_LAYOUT_NHWC = [B,T,dim_f,4] (the network's internal channels-last order).
 */
#ifndef ALSEP_H
#define ALSEP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ALSEP_ABI_VERSION 1

enum { ALSEP_F32 = 0, ALSEP_BF16 = 1, ALSEP_F16 = 2 };
enum { ALSEP_LAYOUT_REF = 0, ALSEP_LAYOUT_NHWC = 1 };
enum {
    ALSEP_OK = 0,
    ALSEP_ERR_ARG = -1,        /* bad argument / unsupported geometry */
    ALSEP_ERR_HIP = -2,        /* a HIP runtime call failed */
    ALSEP_ERR_NOMEM = -3,
    ALSEP_ERR_STATE = -4
};

typedef struct alsep_ctx alsep_ctx;
typedef struct alsep_plan alsep_plan;     /* STFT geometry + twiddle/envelope tables */
typedef struct alsep_net alsep_net;       /* packed TFC-TDF U-Net weights */

int alsep_abi_version(void);

/* ctx: replaces device selection at modules/separator/stem_separator.py:99-100. */
int alsep_create(int device_id, void* hip_stream, alsep_ctx** out);
int alsep_destroy(alsep_ctx* ctx);
const char* alsep_last_error(const alsep_ctx* ctx);

/* Per-kernel-class timing with HIP events recorded on the ctx stream around every launch of
 * the selected class (used by bench.py for the live roofline figure).  begin selects a class,
 * end synchronises, returns the summed kernel time and launch count, and switches timing off. */
enum {
    ALSEP_PROF_NONE = 0,
    ALSEP_PROF_CONV3X3 = 1,      /* conv3x3_bf16_kernel<64> / conv3x3_kernel<...,64>: the plain main-tile kernel */
    ALSEP_PROF_CONV3X3_SMALL = 2,/* conv3x3_kernel, TW<64 tiles (deep levels) */
    ALSEP_PROF_TDF = 3,          /* tdf_gemm_kernel */
    ALSEP_PROF_PIX = 4,          /* pix_gemm_kernel (ds / us) */
    ALSEP_PROF_POINTWISE = 5,    /* first / final 1x1 conv */
    ALSEP_PROF_STFT = 6,
    ALSEP_PROF_ISTFT = 7,
    ALSEP_PROF_CONV3X3_REGW = 8, /* conv3x3_bf16_regw_kernel (persistent, level 0) */
    ALSEP_PROF_CONV3X3_PIPE = 9, /* conv3x3_bf16_pipe_kernel (opt-in) */
    ALSEP_PROF_CONV3X3_BIG = 10, /* conv3x3_bf16_big_kernel<2> (8-wave 8x64 tile, 96 channels: level 1) */
    ALSEP_PROF_CONV3X3_BIG3 = 11,/* conv3x3_bf16_big_kernel<3> (same kernel, 144 channels: level 2) */
    ALSEP_PROF_NN_GEMM = 12,     /* nn_gemm_tn_kernel / nn_bgemm_kernel (float32 MFMA products of the transformer / Demucs / MDX23C families) */
    ALSEP_PROF_NN_CONV = 13,     /* nn_conv2d_tiled_kernel / vr_conv2d_kernel through alsep_nn_conv2d */
    ALSEP_PROF_NN_GEMM_H = 14,   /* nn_gemm_h_kernel (f16 MFMA Linear) */
    ALSEP_PROF_NN_ATTN_H = 15,   /* nn_attn_h_kernel (one-pass f16 attention) */
    ALSEP_PROF_NN_CONV_H = 16,   /* nn_conv_hh_kernel (f16 MFMA convolution) + its split-K reduction */
    ALSEP_PROF_NN_DCONV_H = 17,  /* nn_dconv_h_kernel (f16 MFMA convolution of HTDemucs' half-precision mode) */
    ALSEP_PROF_NN_NORM_H = 18,   /* nn_norm_h_* (GroupNorm / LayerNorm to half: statistics, final, apply) */
    ALSEP_PROF_NN_LSTM = 19,     /* nn_lstm_kernel (the recurrence of HDemucs' BLSTM) */
    ALSEP_PROF_NN_LOCALSTATE = 20,/* nn_localstate_softmax_kernel (HDemucs' LocalState bias / mask / softmax) */
    ALSEP_PROF_PITCH_ANALYSIS = 21,  /* alsep_pitch_shift: gather, forward transforms, polar form, peaks / owners (pv_lock_kernel) */
    ALSEP_PROF_PITCH_RECURRENCE = 22,/* pv_recurrence_kernel */
    ALSEP_PROF_PITCH_SYNTHESIS = 23, /* spectrum, inverse transforms, overlap-add */
    ALSEP_PROF_PITCH_RESAMPLE = 24,  /* pv_resample_kernel */
    ALSEP_PROF_COMPARE_RESAMPLE = 25,/* alsep_resample_fft_f64: pack, the two transforms, the spectrum copy, unpack */
    ALSEP_PROF_COMPARE_RMS = 26,     /* cmp_sumsq_partial_kernel, cmp_sumsq_final_kernel */
    ALSEP_PROF_COMPARE_WAVE = 27,    /* cmp_wave_kernel */
    ALSEP_PROF_COMPARE_SPECTRA = 28, /* cmp_spectra_kernel */
    ALSEP_PROF_COMPARE_REDUCE = 29   /* cmp_minmax_kernel, cmp_colmax_kernel */
};
int alsep_profile_begin(alsep_ctx* ctx, int category);
int alsep_profile_end(alsep_ctx* ctx, double* total_ms, int64_t* launches);
/* arithmetic / minimal HBM traffic of the launches bracketed since alsep_profile_begin, as their launch sites count them (the NN_*
 * categories: 2 M N K per product, operands + result once); call before alsep_profile_end */
int alsep_profile_work(alsep_ctx* ctx, double* flops, double* bytes);
/* Launches of one kernel since alsep_create / alsep_launch_counts_reset, by the name the launch site reports
 * ("conv3x3_bf16_big_kernel<2>", "conv3x3_bf16_regw_kernel", "tdf_bf16_wide_kernel<res>", "us_stream_kernel",
 * "istft_r16_kernel" ...): lets a parity test prove WHICH kernel produced the result it checked.  -1 on a null argument. */
int64_t alsep_launch_count(const alsep_ctx* ctx, const char* kernel);
int alsep_launch_counts_reset(alsep_ctx* ctx);

/* STFT plan: geometry of ConvTDFNetTrim.__init__ (modules/rvc/infer/modules/uvr5/mdxnet.py:15-39).
 * dim_t is the frame count (2**dim_t_arg).  chunk = hop*(dim_t-1). */
int alsep_plan_create(alsep_ctx* ctx, int n_fft, int hop, int dim_f, int dim_t, alsep_plan** out);
int alsep_plan_destroy(alsep_plan* plan);
int alsep_plan_supported_nfft(int n_fft);   /* 1 if an FFT kernel is instantiated for n_fft */

/* STFT: ConvTDFNetTrim.stft (mdxnet.py:41-56): reflect-padded (center=True) periodic-Hann
 * frames, one-sided unnormalised DFT, bins [0,dim_f).
 * Chunk b reads pcm[ch*ch_stride + b*chunk_stride + s], s in [0,chunk): with
 * chunk_stride=gen and ch_stride=len this frames the zero-padded mix of demix_base
 * (mdxnet.py:152-163) in place; with chunk_stride=2*chunk, ch_stride=chunk it is [B,2,chunk]. */
int alsep_stft(alsep_ctx* ctx, const alsep_plan* plan, const float* pcm, int64_t ch_stride,
               int64_t chunk_stride, int64_t n_chunks, void* spec, int dtype, int layout);

/* iSTFT: ConvTDFNetTrim.istft (mdxnet.py:58-75): zero bins >= dim_f, inverse DFT, window,
 * overlap-add, divide by sum w^2, drop n_fft/2 each side.  Sample s of chunk b, with
 * keep_lo <= s < keep_hi, is written to out[ch*out_ch_stride + b*out_chunk_stride + (s-keep_lo)]
 * if that offset < out_limit.  keep=[0,chunk), strides (chunk, 2*chunk) give [B,2,chunk];
 * keep=[trim,chunk-trim), out_chunk_stride=gen stitches demix_base's output
 * (mdxnet.py:178-183) directly. */
int alsep_istft(alsep_ctx* ctx, const alsep_plan* plan, const void* spec, int dtype, int layout,
                int64_t n_chunks, float* out, int64_t out_ch_stride, int64_t out_chunk_stride,
                int64_t keep_lo, int64_t keep_hi, int64_t out_limit);

/* Hann-window overlap-add chunker of the third-party MDXSeparator.demix (what Separator.separate runs
 * today, stem_separator.py:281; package audio-separator>=0.32.0, setup.sh:96 -- PARITY UNPINNED):
 * chunks [n_chunks,2,chunk] are the model outputs of windows starting every `step` samples of the padded
 * mixture of length `total`; out[c*out_stride + i] = gain * sum_b w_b y_b / sum_b w_b at mixture position
 * p_lo + i, w_b = np.hanning(min(chunk, total - b*step)) (or 1 when use_window == 0). */
int alsep_ola_combine(alsep_ctx* ctx, const float* chunks, int64_t n_chunks, int64_t chunk, int64_t step,
                      int64_t total, int use_window, float gain, float* out, int64_t out_stride, int64_t p_lo,
                      int64_t n_out);
/* The same overlap-add split over the ranks of a job: `chunks` holds only the chunks [b0, b1) of this rank; part [3][n_out] =
 * raw weighted sums of the two channels and the summed weights over those chunks.  The ranks' parts are SUMMED by one collective (at a
 * shard seam chunks of two ranks overlap), then alsep_ola_finish divides: out[c][i] = gain * part[c][i] / part[2][i]. */
int alsep_ola_partial(alsep_ctx* ctx, const float* chunks, int64_t b0, int64_t b1, int64_t chunk, int64_t step, int64_t total,
                      int use_window, float* part, int64_t p_lo, int64_t n_out);
int alsep_ola_finish(alsep_ctx* ctx, const float* part, float gain, float* out, int64_t out_stride, int64_t n_out);
/* Sample-rate conversion of rows of PCM, x [rows, n_in] at sr_in -> y [rows, n_out] at sr_out (n_out = ceil(n_in * sr_out / sr_in) as
 * librosa): what librosa.load(path, sr=44100) does to a 48 kHz input at modules/separator/stem_separator.py:865.  The reference uses
 * libsoxr there (not in /root/reference): this is the build's own Kaiser-windowed sinc (`zeros` zero crossings per side, cut-off
 * rolloff * min(sr_in, sr_out) / 2, Kaiser beta) -- PARITY UNPINNED; restated in oracle/mdx_oracle.py resample(). */
int alsep_resample(alsep_ctx* ctx, const float* x, float* y, int64_t rows, int64_t n_in, int64_t n_out, int sr_in, int sr_out,
                   int zeros, float rolloff, float beta);
/* scipy.signal.resample_poly(x, up, down) with a caller-made filter (its default: firwin(20 max(up, down) + 1, 1 / max(up, down),
 * window=("kaiser", 5.0)) * up in float32) -- what librosa.resample(res_type="polyphase") runs in the VR band chain going down
 * (modules/rvc/infer/modules/uvr5/vr.py:74-79, modelparams/4band_v*.json "res_type").  up / down already divided by their gcd;
 * n_pre_pad = down - half_len % down, n_pre_remove = (half_len + n_pre_pad) / down, n_out = ceil(n_in up / down) as scipy computes
 * them (audiolab_amd/vr_frontend.py).  x [rows, n_in] -> y [rows, n_out], taps on the device. */
int alsep_resample_poly(alsep_ctx* ctx, const float* x, float* y, int64_t rows, int64_t n_in, int64_t n_out, int up, int down,
                        const float* taps, int n_taps, int n_pre_pad, int n_pre_remove);
/* scipy.signal.resample(x, n_out) (Fourier method) -- librosa.resample(res_type="scipy"), the VR band chain going up
 * (modules/rvc/infer/lib/uvr5_pack/lib_v5/spec_utils.py:427): spectrum truncated / zero-padded with scipy's Nyquist rule, inverse
 * transform times n_out / n_in.  Any lengths <= 2^27 (float64 Bluestein transforms); rows go two per complex transform. */
int64_t alsep_resample_fft_workspace_bytes(int64_t n_in, int64_t n_out);
int alsep_resample_fft(alsep_ctx* ctx, const float* x, int64_t ldx, float* y, int64_t ldy, int64_t rows, int64_t n_in, int64_t n_out,
                       void* ws, int64_t ws_bytes);
/* the same on float64 rows (the Compare chain below): no rounding to single precision on the way */
int64_t alsep_resample_fft_f64_workspace_bytes(int64_t n_in, int64_t n_out);
int alsep_resample_fft_f64(alsep_ctx* ctx, const double* x, int64_t ldx, double* y, int64_t ldy, int64_t rows, int64_t n_in, int64_t n_out,
                           void* ws, int64_t ws_bytes);
/* zero the lowest nbins bins of a spectrogram in place (MDXSeparator.run_model zeroes bins 0..2). */
int alsep_zero_low_bins(alsep_ctx* ctx, void* spec, int dtype, int layout, int64_t B, int64_t dim_f, int64_t T,
                        int nbins);

/* Spectrogram layout conversion REF <-> NHWC (same dtype). */
int alsep_spec_convert(alsep_ctx* ctx, const void* src, void* dst, int dtype, int src_layout,
                       int64_t B, int64_t dim_f, int64_t T);

/* TFC-TDF U-Net ("ConvTDFNet", the network inside the *.onnx models loaded at
 * stem_separator.py:394,512 and run through MDXSeparator.model_run,
 * handlers/patch_separate.py:52,58-62).
 * Weights arrive as a table of named fp32 device tensors in torch state_dict layout with
 * BatchNorm already folded to per-channel (scale, shift) by the caller; the library
 * repacks them into MFMA fragment order in its own memory. */
typedef struct alsep_net_config {
    int32_t dim_f;        /* frequency bins in/out */
    int32_t dim_t;        /* frames */
    int32_t num_blocks;   /* L (11): n = L/2 encoder and decoder levels + bottleneck */
    int32_t l;            /* convs per TFC block */
    int32_t g;            /* channel growth */
    int32_t bn;           /* TDF bottleneck factor (f -> f/bn -> f); 0 = single f->f linear */
    int32_t dtype;        /* ALSEP_F32 | ALSEP_BF16 | ALSEP_F16 */
    int32_t flags;        /* 0, or ALSEP_NET_SPLIT_F16 (float32 networks only) */
} alsep_net_config;
/* float32 storage with the contractions (3x3 convolutions, ds / us, TDF linears) on the 16-bit matrix pipe: every float32 operand is
 * carried as two IEEE halves (hi, scaled lo) and a product costs three f16 MFMAs accumulated in float32 -- 2^-22 relative per product,
 * the float32 mode's accuracy at 5 x its matrix throughput; activations must stay inside the half range (|x| <= 65504), beyond it the
 * outputs are Inf / NaN.  Without the flag a float32 network runs on v_mfma_f32_16x16x4_f32 (exact fmaf chains). */
#define ALSEP_NET_SPLIT_F16 1

typedef struct alsep_tensor {
    const char* name;     /* e.g. "encoding_blocks.0.tfc.H.1.0.weight", "...scale", "...shift" */
    const float* data;    /* device pointer, fp32, contiguous */
    int64_t numel;
} alsep_tensor;

int alsep_net_create(alsep_ctx* ctx, const alsep_net_config* cfg, const alsep_tensor* tensors,
                     int64_t n_tensors, alsep_net** out);
int alsep_net_destroy(alsep_net* net);
/* bytes of caller-provided scratch for a batch of B chunks */
int64_t alsep_net_workspace_bytes(const alsep_net* net, int64_t B);
/* spec_in/spec_out: [B,T,dim_f,4] (NHWC) in the net's dtype.
 *   spec_out = out_alpha * net(in_scale * spec_in) + out_beta * spec_out
 * (in_scale=1, alpha=1, beta=0: plain forward; the denoise average of mdxnet.py:168-173,
 * 0.5*f(x) - 0.5*f(-x), is two calls: (1, 0.5, 0) then (-1, -0.5, 1)). */
int alsep_net_forward(alsep_ctx* ctx, const alsep_net* net, const void* spec_in, void* spec_out,
                      int64_t B, void* workspace, int64_t workspace_bytes, float in_scale,
                      float out_alpha, float out_beta);
/* alsep_stft (channels-last, the network's storage type) + alsep_net_forward in one call for the half-precision networks: the STFT and
 * the network's first 1x1 convolution run as ONE kernel (no spectrogram in HBM), bit-identical to the two calls.  pcm / ch_stride /
 * chunk_stride as alsep_stft; zero_low_bins: bins below it enter the network as zeros (alsep_zero_low_bins of the overlap-add runner).
 * Returns ALSEP_ERR_STATE when this (plan, network) pair has no fused kernel: call alsep_stft + alsep_net_forward then. */
int alsep_net_forward_pcm(alsep_ctx* ctx, const alsep_net* net, const alsep_plan* plan, const float* pcm, int64_t ch_stride,
                          int64_t chunk_stride, void* spec_out, int64_t B, void* workspace, int64_t workspace_bytes, float in_scale,
                          float out_alpha, float out_beta, int zero_low_bins);

/* The generic float32 GEMM / convolution entry points (alsep_nn_bgemm*, alsep_nn_conv2d, alsep_vr_conv2d on their tiled paths) of THIS
 * context: split = 1 runs their contractions as split-half products on the f16 matrix pipe (float32 in and out, 2^-22 per product,
 * operands limited to the half range), split = 0 (default) on exact f32 MFMA.  Call outside a stream capture. */
int alsep_nn_set_contraction(alsep_ctx* ctx, int split);
/* *out = 1 when a split-contraction launch of this context met an operand beyond the half range since the last call (results since then
 * are invalid: run them again with split = 0).  Reads and clears the word; synchronises ctx's stream. */
int alsep_nn_range_flag(alsep_ctx* ctx, int32_t* out);

/* ALSEP_NET_SPLIT_F16 networks: *out = 1 when any forward since the last call met an operand beyond the half range (|x| > 65504, or not
 * a number) -- the results of those forwards are invalid (rebuild the network without the flag for such input).  Reads and clears the
 * network's range word; synchronises ctx's stream.  *out = 0 for every other network. */
int alsep_net_range_flag(alsep_ctx* ctx, alsep_net* net, int32_t* out);

/* Element-wise / reduction ops of the ensemble stage (stem_separator.py:241-262,173-239,
 * 415-456) and of the MDX runner (mdxnet.py:168-173 denoise average, :211 secondary stem). */
/* y = a*x + b*y over n floats */
int alsep_axpby(alsep_ctx* ctx, float a, const float* x, float b, float* y, int64_t n);
/* out[0] = max |x| (out is a device float; written, not accumulated) */
int alsep_peak_abs(alsep_ctx* ctx, const float* x, int64_t n, float* out);
/* y *= s where s is read from a device float: y = y * (num / max(*den, floor)) */
int alsep_scale_by_device(alsep_ctx* ctx, float* y, int64_t n, float num, const float* den, float floor_);
/* dots[0..2] = <a,b>, <a,a>, <b,b> in double precision.  dots must hold 4 + 3*1024 device
 * doubles: [0..2] results, [4..] per-block partials (deterministic two-stage sum). */
int alsep_dot3(alsep_ctx* ctx, const float* a, const float* b, int64_t n, double* dots);
/* corr[j] = sum_n ref[n+lag]*sig[n], lag = j - max_shift, over the first `probe` samples
 * (np.correlate(ref[:probe], sig[:probe], "full") centre window, stem_separator.py:216-224) */
int alsep_xcorr_window(alsep_ctx* ctx, const float* ref, const float* sig, int64_t probe,
                       int max_shift, double* corr);
/* out[n] = ref[n] - alpha * sig[n-lag] (zero outside), n in [0,len) (stem_separator.py:196-232) */
int alsep_shift_subtract(alsep_ctx* ctx, const float* ref, const float* sig, int64_t len, int lag,
                         float alpha, float* out);

/* ---- VR-architecture building blocks (CascadedASPPNet: reference modules/rvc/infer/lib/uvr5_pack/lib_v5/nets*.py,
 * layers*.py).  Channels-last float32 tensors [B, H = bins, W = frames, C].  Outputs that feed a
 * torch.cat are written into the channel slice [y_coff, y_coff + C) of a tensor with y_ctotal channels. ---- */
/* y = act(conv2d(x, w) * scale + shift): nn.Conv2d(bias=False) + folded BatchNorm2d + activation (layers*.py:9-27);
 * w packed [KH][KW][Cin][Cout]; act 0 none, 1 ReLU, 2 LeakyReLU(0.01); padding / dilation per axis (layers_new.py:83-91 uses
 * (4,2), (8,4), (12,6)).  Output size as torch: (H + 2 pad_h - dil_h (KH-1) - 1) / stride + 1.  A Linear (+ bias, BatchNorm1d)
 * is the 1x1 case with the rows as pixels. */
int alsep_vr_conv2d(alsep_ctx* ctx, const float* x, const float* w, const float* scale, const float* shift, float* y,
                    int64_t B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad_h, int pad_w, int dil_h,
                    int dil_w, int act, int y_ctotal, int y_coff);
/* recurrent part of one direction of nn.LSTM (layers_new.py:117-121): pre [T,N,4*hidden] = x W_ih^T + b_ih + b_hh (gates
 * i,f,g,o), whh [4*hidden][hidden]; h_t is written to out[t, n, out_off .. out_off+hidden) of rows out_stride wide;
 * reverse != 0 walks t from T-1 down (the backward direction).  hidden in {16, 32, 64}. */
int alsep_vr_lstm(alsep_ctx* ctx, const float* pre, const float* whh, float* out, int T, int N, int hidden, int out_stride,
                  int out_off, int reverse);
/* depthwise (groups = C) KHxKW dilated convolution, same-size output (layers*.py:30-52); w packed [C][KH][KW] */
int alsep_vr_depthwise(alsep_ctx* ctx, const float* x, const float* w, float* y, int64_t B, int H, int W, int C, int KH, int KW,
                       int pad, int dil);
/* F.interpolate(mode="bilinear", align_corners=True) to (Ho, Wo) (layers*.py:84, 111) */
int alsep_vr_resize_bilinear(alsep_ctx* ctx, const float* x, float* y, int64_t B, int H, int W, int C, int Ho, int Wo,
                             int y_ctotal, int y_coff);
/* spec_utils.crop_center (spec_utils.py:12-27) + concat: y[bh, wq, y_coff + c] = x[bh, w_off + wq, c]; BH = B * H rows */
int alsep_vr_copy_slice(alsep_ctx* ctx, const float* x, float* y, int64_t BH, int Wx, int C, int w_off, int Wy, int y_ctotal,
                        int y_coff);
/* nn.AdaptiveAvgPool2d((1, None)) (layers*.py:93): mean over bins -> [B, 1, W, C] */
int alsep_vr_mean_h(alsep_ctx* ctx, const float* x, float* y, int64_t B, int H, int W, int C);
/* nets*.py:80-111: mask = sigmoid(logit) replicate-padded from Hm to Hout bins, mask ** (1 + a/3) below split_bin and
 * ** (1 + a) from it on when aggressiveness a >= 0, out = mask * mix */
int alsep_vr_mask(alsep_ctx* ctx, const float* logit, const float* mix, float* out, int64_t B, int Hm, int Hout, int W, int C,
                  int split_bin, float aggressiveness);

/* ---- Demucs family (HTDemucs: what audio_separator's DemucsSeparator runs for htdemucs_6s.yaml, loaded at
 * modules/separator/stem_separator.py:466 and run at :479; network source in the un-vendored demucs>=4.0.1, requirements.txt:19 --
 * PARITY UNPINNED).  Generic channels-last float32 building blocks; activations: 0 none, 1 ReLU, 2 LeakyReLU(0.01), 3 GELU (erf),
 * 4 GLU over the channel axis (C -> C/2; norm / act only). ---- */
/* alsep_vr_conv2d with a stride per axis and GELU: Conv1d over [B,L,C] is the W = 1 case, a Linear the 1x1 case */
int alsep_nn_conv2d(alsep_ctx* ctx, const float* x, const float* w, const float* scale, const float* shift, float* y, int64_t B, int H,
                    int W, int Cin, int Cout, int KH, int KW, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h, int dil_w,
                    int act, int y_ctotal, int y_coff);
/* C[b1,b2][m][n] = alpha * sum_k A[b1,b2][m][k] B[b1,b2][n][k]; sa / sb / sc = element strides {b1, b2, row, k-or-column} (the
 * attention products of nn.MultiheadAttention straight from the packed in-projection, no head transposes) */
int alsep_nn_bgemm(alsep_ctx* ctx, const float* A, const float* B, float* C, int nb1, int nb2, int M, int N, int K, const int64_t* sa,
                   const int64_t* sb, const int64_t* sc, float alpha);
/* softmax over the last dimension of x [rows, n], in place */
int alsep_nn_softmax_rows(alsep_ctx* ctx, float* x, int64_t rows, int n);
/* the same on rows `ld` floats apart (a score matrix whose rows are padded to a multiple of 4 floats) */
int alsep_nn_softmax_rows_ld(alsep_ctx* ctx, float* x, int64_t rows, int n, int ld);
/* bytes of device scratch (8-byte aligned) for alsep_nn_norm / alsep_nn_meanstd over G groups of per_group elements */
int64_t alsep_nn_stats_workspace_bytes(int64_t G, int64_t per_group);
/* x [G, R, C]: normalise every group of R rows x C channels to zero mean / unit (biased) variance, y = act(n * gamma[c] + beta[c]):
 * nn.GroupNorm(1, C) (R = positions of one sample), nn.LayerNorm(C) (R = 1), demucs MyGroupNorm (R = tokens).  gamma / beta may
 * both be NULL.  act 0, 3 or 4. */
int alsep_nn_norm(alsep_ctx* ctx, const float* x, float* y, const float* gamma, const float* beta, int64_t G, int64_t R, int C, float eps,
                  int act, void* workspace);
/* stats[2 s] = mean, stats[2 s + 1] = UNBIASED std of sample s (HTDemucs.forward: mean / std of the whole spectrogram / waveform) */
int alsep_nn_meanstd(alsep_ctx* ctx, const float* x, int64_t nsamples, int64_t per_sample, float* stats, void* workspace);
/* inverse 0: y = (x - mean) / (eps + std); inverse 1: y = x * std + mean */
int alsep_nn_affine_stats(alsep_ctx* ctx, const float* x, float* y, const float* stats, int64_t nsamples, int64_t per_sample, float eps,
                          int inverse);
/* y = act(x) over x [rows, C]; act 1, 3 or 4 */
int alsep_nn_act(alsep_ctx* ctx, const float* x, float* y, int64_t rows, int C, int act);
/* y = a + scale[c] * b (LayerScale residual; scale NULL: plain add) */
int alsep_nn_scale_add(alsep_ctx* ctx, const float* a, const float* b, const float* scale, float* y, int64_t rows, int C);
/* y[i] += s * e[((i / inner) % period) * C + i % C]: frequency embedding over [B,F,T,C] (inner = T*C, period = F), positional
 * embedding over [B,N,C] (inner = C, period = N) */
int alsep_nn_add_bcast(alsep_ctx* ctx, float* y, const float* e, float s, int64_t n, int64_t inner, int period, int C);
/* y[r * y_stride + i] += w[i] * x[r * x_stride + i], i < n (triangular overlap-add of demucs.apply.apply_model);  y[r][i] /= w[i] */
int alsep_nn_vec_fma(alsep_ctx* ctx, float* y, const float* x, const float* w, int64_t rows, int64_t n, int64_t y_stride, int64_t x_stride);
int alsep_nn_vec_div(alsep_ctx* ctx, float* y, const float* w, int64_t rows, int64_t n);
/* y [B, L, C] = x [B, C, L] (waveform [B,2,L] <-> channels-last [B,L,2]) */
int alsep_nn_swap_last2(alsep_ctx* ctx, const float* x, float* y, int64_t B, int64_t C, int64_t L);
/* F.pad(mode="reflect") along the last axis: [rows, n] -> [rows, left + n + right] */
int alsep_nn_reflect_pad(alsep_ctx* ctx, const float* x, float* y, int64_t rows, int64_t n, int64_t left, int64_t right);
/* second half of ConvTranspose([K,1], stride [S,1]), K = 2 S: g [B, I, J, K*Cout] = 1x1 conv of the input with the weights packed
 * [Cin][k*Cout + co]; y [B, Lout, J, Cout] = act(g[i][r] + g[i-1][r+S] + bias), o + pad = i S + r (the crop of HDecLayer.forward) */
int alsep_nn_tconv_fold(alsep_ctx* ctx, const float* g, const float* bias, float* y, int64_t B, int I, int J, int Cout, int S, int pad,
                        int Lout, int act);
/* spec [B,4,F,Tt] (alsep_stft, reference layout) -> y [B,F,T,4] = scale * spec[..., t_off : t_off + T]   (HTDemucs._spec/_magnitude) */
int alsep_demucs_spec_in(alsep_ctx* ctx, const float* spec, float* y, int64_t B, int F, int Tt, int T, int t_off, float scale);
/* x [B,F,T,S*4] (normalised output), stats of the input spectrogram -> spec [B*S,4,F,Tt]: frames [t_off, t_off+T) =
 * scale * (x * std + mean), the rest zero   (HTDemucs._mask with cac + the frame padding of _ispec) */
int alsep_demucs_spec_out(alsep_ctx* ctx, const float* x, const float* stats, float* spec, int64_t B, int S, int F, int Tt, int T,
                          int t_off, float scale);
/* out [B,S,2,L] = (xt [B,L,S*2] * stdt + meant) + xs [B*S,2,L]   (the last lines of HTDemucs.forward) */
int alsep_demucs_mix_out(alsep_ctx* ctx, const float* xt, const float* statst, const float* xs, float* out, int64_t B, int S, int64_t L);
/* ---- HDemucs (csrc/nn_hdemucs.h) ----
 * One bidirectional LSTM layer's recurrence (torch.nn.LSTM, gate order i, f, g, o), both directions and all N sequences in ONE launch:
 *   pre [T, N, 8H] = x W_ih^T + b_ih + b_hh of the forward (columns 0 .. 4H) and the reverse direction (4H .. 8H);
 *   whh_t [2, H, 4H] = W_hh^T of each direction (forward first);  h [T, N, 2H] = h_t, forward direction in the first H columns.
 * Zero initial state.  16 <= H <= 512, H % 16 == 0. */
int alsep_nn_lstm(alsep_ctx* ctx, const float* pre, const float* whh_t, float* h, int T, int N, int H);
/* demucs LocalState between its two products, in place over scores [B*heads, T, ld] (rows: queries s, columns: keys t, already scaled):
 * adds -sum_f (f+1) |t - s| / sqrt(nd) * sigmoid(qd[b, s, h*nd + f]) / 2, sets the diagonal to -100, softmax over t.
 * qd: the query_decay projection, channels-last rows of qd_ld floats. */
int alsep_nn_localstate_softmax(alsep_ctx* ctx, float* scores, const float* qd, int64_t B, int heads, int T, int ld, int nd, int64_t qd_ld);
/* demucs BLSTM framing.  unfold: x [B, T, C] -> frames [width, B*nf, C], frames[w][b*nf + k] = x[b][k*stride + w] (zero beyond T).
 * stitch: y [B, T, C] = skip + frames[t - k*stride][b*nf + k] with k = clamp((t - stride/2) / stride, 0, nf - 1); nf == 1: no framing. */
int alsep_nn_blstm_unfold(alsep_ctx* ctx, const float* x, float* frames, int64_t B, int T, int C, int width, int stride, int nf);
int alsep_nn_blstm_stitch(alsep_ctx* ctx, const float* frames, const float* skip, float* y, int64_t B, int T, int C, int width, int stride,
                          int nf);
/* nn.GroupNorm(G, C) over channels-last x [B, R, C], then act 0, 3 (GELU) or 4 (GLU); writes rows [r0, r0 + Ro) of each sample into
 * y [B, Ro, C'] (the crop of HDecLayer after its norm2).  stats: 2 B G floats of device scratch. */
int alsep_nn_group_norm(alsep_ctx* ctx, const float* x, float* y, const float* gamma, const float* beta, int64_t B, int R, int C, int G,
                        float eps, int act, int r0, int Ro, float* stats);
/* a bag of Demucs models, last step: V views (one shift pass of one member each) -> the stems out [S,2,L] in one pass,
 *   out[s,c,t] = stats[0] + stats[1] * sum_v coef[v*S+s] * q_v(row[v*S+s]*2 + c, t + cut[v]),
 *   q_v(r, x) = wsum[v][x] != 0 ? acc[v][r * ld[v] + x] / wsum[v][x] : 0;  row[v*S+s] < 0: view v does not carry source s.
 * Every array is device memory: acc / wsum hold V device pointers, ld (int64) and cut (int32) V entries, row (int32) and coef V*S.
 * The caller guarantees 0 <= cut[v], cut[v] + L <= ld[v] and that wsum[v] holds cut[v] + L values.  1 <= S <= 8, 1 <= V <= 64. */
int alsep_demucs_bag_finish(alsep_ctx* ctx, const float* const* acc, const float* const* wsum, const int64_t* ld, const int32_t* cut,
                            const int32_t* row, const float* coef, const float* stats, float* out, int V, int S, int64_t L);

/* ---- Roformer family (BS-RoFormer / Mel-Band RoFormer: the first members of the reference's default ensemble and its de-reverb /
 * de-echo models, stem_separator.py:379-382, 796-797; network source in the un-vendored audio-separator -- PARITY UNPINNED).  Further
 * building blocks on the same channels-last float32 tensors; activation 5 = tanh. ---- */
/* alsep_nn_bgemm with an epilogue: C = act(alpha * A B^T + bias[column]); bias may be NULL; act 0, 3 (GELU) or 5 (tanh) */
int alsep_nn_bgemm_bias(alsep_ctx* ctx, const float* A, const float* B, float* C, int nb1, int nb2, int M, int N, int K, const int64_t* sa,
                        const int64_t* sb, const int64_t* sc, float alpha, const float* bias, int act);
/* RMSNorm over the last axis: y = x / max(||x||, 1e-12) * sqrt(C) * gamma; rows at x + r * x_stride / y + r * y_stride (a column slice of a
 * wider matrix in place when both strides are its width) */
int alsep_nn_rmsnorm(alsep_ctx* ctx, const float* x, float* y, const float* gamma, int64_t rows, int C, int64_t x_stride, int64_t y_stride);
/* rotary position embedding (interleaved pairs, theta 10000) in place on the heads * d columns from col_off of every row of x
 * [rows, row_stride]; position of row r = (r / pos_div) % pos_mod */
int alsep_nn_rotary(alsep_ctx* ctx, float* x, int64_t rows, int64_t row_stride, int col_off, int heads, int d, int64_t pos_div, int64_t pos_mod);
/* out [rows, heads * d] *= sigmoid(gates [rows, heads]) per head */
int alsep_nn_gate(alsep_ctx* ctx, float* out, const float* gates, int64_t rows, int heads, int d);
/* band-split input: feat [T, 2 * n_idx], feat[t, 2 i + c] = spec[(s*2 + c), f, t] with midx[i] = 2 f + s (spec [4, F, T] from alsep_stft) */
int alsep_roformer_gather(alsep_ctx* ctx, const float* spec, const int* midx, float* feat, int n_idx, int F, int T);
/* mask estimator output h [T, H] -> complex masks (GLU, averaged over the bands that cover a bin: occurrences occ_start[m] .. occ_start[m+1]
 * with value columns col_a[o], col_a[o]+1 and gate columns col_g[o], col_g[o]+1), out = spec * mask, same [4, F, T] layout */
int alsep_roformer_mask(alsep_ctx* ctx, const float* spec, const float* h, const int* occ_start, const int* col_a, const int* col_g,
                        float* out, int F, int T, int H);

/* ---- MDX23C (TFC-TDF v3: ensemble slot 4 and the drum-kit splitter, stem_separator.py:383, 541; network source in the un-vendored
 * audio-separator -- PARITY UNPINNED).  Further building blocks. ---- */
/* nn.InstanceNorm2d(affine) on channels-last x [P, C] (one sample): per-channel statistics over the P pixels, y = act(n * gamma + beta);
 * act 0 or 3 (GELU); gamma / beta may both be NULL */
int64_t alsep_nn_instnorm_workspace_bytes(int64_t P, int C);
int alsep_nn_instnorm(alsep_ctx* ctx, const float* x, float* y, const float* gamma, const float* beta, int64_t P, int C, float eps, int act,
                      void* workspace);
/* the same with y stored as IEEE half (C % 4 == 0): the activation a half-precision convolution reads (MDX23C's half-precision mode --
 * stem_separator.py:106 use_autocast=True: convolutions in half, normalisation in float32) */
int alsep_nn_instnorm_f16(alsep_ctx* ctx, const float* x, void* y, const float* gamma, const float* beta, int64_t P, int C, float eps, int act,
                          void* workspace);
/* the same for x [T][F][C] with the half result stored [T][C][F] (frequency-contiguous rows per frame and channel): the operand layout
 * of the TDF Linear over the frequency axis as one batched alsep_nn_gemm_f16 per frame (A = the shared weight matrix) */
int alsep_nn_instnorm_f16_t(alsep_ctx* ctx, const float* x, void* y, const float* gamma, const float* beta, int64_t T, int F, int C, float eps,
                            int act, void* workspace);
/* Conv2d on v_mfma_f32_16x16x32_f16: x IEEE half channels-last [B, H, W, Cin], w IEEE half [Cout][KH][KW][Cin], float32 result into the
 * channel slice [y_coff, y_coff + Cout) of y [B, Ho, Wo, y_ctotal], optionally + R (float32 [pixels][ldr]: a block's shortcut branch).
 * Cin % 64 == 0, Cout % 4 == 0; no bias, no activation (this network has neither after a convolution).  Layers with few output tiles are
 * split along K (partial tiles in `workspace`, summed in a fixed order): alsep_nn_conv2d_f16_workspace_bytes says how much they need. */
int64_t alsep_nn_conv2d_f16_workspace_bytes(int64_t B, int H, int W, int Cin, int Cout, int KH, int KW, int stride_h, int stride_w, int pad_h,
                                            int pad_w);
int alsep_nn_conv2d_f16(alsep_ctx* ctx, const void* x, const void* w, float* y, const float* R, int64_t ldr, int64_t B, int H, int W, int Cin,
                        int Cout, int KH, int KW, int stride_h, int stride_w, int pad_h, int pad_w, int y_ctotal, int y_coff, void* workspace,
                        int64_t workspace_bytes);
/* y = a * b element-wise */
int alsep_nn_mul(alsep_ctx* ctx, const float* a, const float* b, float* y, int64_t n);
/* second half of ConvTranspose2d(kernel = stride = 2): g [H, W, 4*Cout] (1x1 conv, columns (dy*2+dx)*Cout + co) -> channel slice
 * [y_coff, y_coff + Cout) of y [2H, 2W, y_ctotal] */
int alsep_nn_depth_to_space2(alsep_ctx* ctx, const float* g, float* y, int H, int W, int Cout, int y_ctotal, int y_coff);
/* spec [4, f*k, T] (alsep_stft) -> x [T, f, 4k], x[t, ff, c2*k + kk] = spec[c2, kk*f + ff, t] (STFT + cac2cws of tfc_tdf_v3);
 * y [T, f, S*4k] -> spec [S, 4, f*k, T] (cws2cac) */
int alsep_mdx23c_spec_in(alsep_ctx* ctx, const float* spec, float* x, int f, int k, int T);
int alsep_mdx23c_spec_out(alsep_ctx* ctx, const float* y, float* spec, int S, int f, int k, int T);

/* ---- VR multi-band front / back end (in-tree reference: modules/rvc/infer/lib/uvr5_pack/lib_v5/spec_utils.py, modules/rvc/infer/modules/uvr5/
 * vr.py:43-196).  Complex spectrograms are float2-interleaved [2, bins, frames]; band spectrograms from / for alsep_stft / alsep_istft are
 * [4 = (L_re, L_im, R_re, R_im), Fb, Tb]. ---- */
/* out[c, o0 + i, t] = gain[i] * band[c, f0 + i, t0 + t] (i < h, t < l; gain may be NULL): combine_spectrograms (:95-125) and the high-end crop */
int alsep_vr_band_crop(alsep_ctx* ctx, const float* band, float* out, const float* gain, int Fb, int Tb, int f0, int t0, int h, int l,
                       int out_bins, int o0);
/* y = pred * exp(i angle X), v = X - y over n complex values (vr.py:110-111) */
int alsep_vr_split_pred(alsep_ctx* ctx, const float* pred, const float* X, float* y, float* v, int64_t n);
/* spec_utils.mirroring("mirroring") (:453-470): spec_m [2, bins, l], he / out [2, hh, l], lo = pre_filter_start - 10 - hh */
int alsep_vr_mirror(alsep_ctx* ctx, const float* spec_m, const float* he, float* out, int bins, int hh, int l, int lo);
/* one band's spectrogram for the iSTFT (cmb_spectrogram_to_wave :353-429): bins [o0, o0+h) of spec_m at [f0, f0+h), then `extra` [2, eh, l]
 * at [e0, e0+eh) (NULL: none), all times gain[f] (the low-pass / high-pass ramps and zeroed ranges), zero elsewhere; band [4, Fb, l] */
int alsep_vr_band_spec(alsep_ctx* ctx, const float* spec_m, const float* extra, const float* gain, float* band, int bins, int l, int Fb, int f0,
                       int h, int o0, int e0, int eh);

/* ---- half-precision MFMA path of the transformer model families (csrc/nn_half.hip): what torch autocast does to the Linear layers and
 * the attention of the Roformer models the reference loads with use_autocast=True (modules/separator/stem_separator.py:106, :379-382).
 * The residual stream and all statistics are float32; whatever a Linear or the attention reads is IEEE half in HBM, written in that
 * type by its producer; products on the f16 MFMA with float32 accumulation. */
int alsep_nn_to_f16(alsep_ctx* ctx, const float* x, void* y, int64_t n);
/* y[r][C] (half) = lucidrains RMSNorm of x[r][C] (float32) times gamma; strides in elements */
int alsep_nn_rmsnorm_f16(alsep_ctx* ctx, const float* x, void* y, const float* gamma, int64_t rows, int C, int64_t x_stride, int64_t y_stride);
/* C[b][M][N] = act(alpha A[b][M][K] W[b][N][K]^T + bias[b][N]) (+ R[b][M][N]); A, W half; C half (c_f16 != 0) or float32; bias, R float32;
 * row strides ld*, batch strides s*_b in elements (0: shared).  act 0 none, 3 GELU(erf), 5 tanh.  Needs K % 8 == 0, N % 4 == 0 and aligned
 * rows (ALSEP_ERR_ARG otherwise).  n_per_batch (device, optional): columns of batch b (<= N). */
int alsep_nn_gemm_f16(alsep_ctx* ctx, const void* A, int64_t lda, int64_t sa_b, const void* W, int64_t ldw, int64_t sw_b, void* C, int c_f16,
                      int64_t ldc, int64_t sc_b, const float* bias, int64_t bias_b, const float* R, int64_t ldr, int64_t sr_b, int nb, int M,
                      int N, int K, float alpha, int act, const int* n_per_batch);
/* out (half) = softmax(scale q k^T) v per (sequence, head), one pass (no score matrix in HBM).  qkv: half rows of 3 * heads * 64 values
 * (q | k | v); sequence s = L rows `row_stride` elements apart from s * seq_stride; out rows of heads * 64.  rot_table (optional,
 * alsep_nn_rotary_table): q and k are rotary-embedded by their position as they are loaded; gates (optional, float32): the result is
 * scaled by sigmoid(gates[seq * g_seq_stride + row * g_row_stride + head]). */
int alsep_nn_attention_f16(alsep_ctx* ctx, const void* qkv, void* out, int n_seq, int L, int heads, int dim_head, int64_t seq_stride,
                           int64_t row_stride, int64_t o_seq_stride, int64_t o_row_stride, float scale, const float* rot_table,
                           const float* gates, int64_t g_seq_stride, int64_t g_row_stride);
/* HTDemucs half-precision mode (csrc/nn_demucs_h.h).
 * Convolution on the f16 matrix pipe for Demucs geometries: x channels-last [B, Hv, W, x_ld] (x_f16: IEEE half, else float32 rounded to
 * half as it is read; rows Hv .. H - 1 of an image read as zeros), w [Cout][Kp] IEEE half, k = (dy, dx, ci) zero-padded from KH KW Cin to
 * Kp (a multiple of 32); y [B, Ho, Wo] pixels y_ld elements apart = act(conv + bias), act 0 or 3 (GELU), half (y_f16) or float32. */
int alsep_nn_conv_h(alsep_ctx* ctx, const void* x, int x_f16, const void* w, const float* bias, void* y, int y_f16, int64_t y_ld, int64_t B,
                    int H, int Hv, int W, int x_ld, int Cin, int Cout, int Kp, int KH, int KW, int stride_h, int stride_w, int pad_h, int pad_w,
                    int dil_h, int dil_w, int act);
/* bytes of device scratch (8-byte aligned) for alsep_nn_norm_h over G groups of per_group elements */
int64_t alsep_nn_norm_h_workspace_bytes(int64_t G, int64_t per_group);
/* alsep_nn_norm with the result stored as IEEE half (y_f16) or float32; the statistics of a group do not depend on G */
int alsep_nn_norm_h(alsep_ctx* ctx, const float* x, void* y, int y_f16, const float* gamma, const float* beta, int64_t G, int64_t R, int C,
                    float eps, int act, void* workspace);
/* cross-attention in half: q [n_seq][Lq] rows, kv [n_seq][Lk] rows of k (heads x 64) | v (heads x 64); out [n_seq][Lq] rows, IEEE half */
int alsep_nn_xattention_f16(alsep_ctx* ctx, const void* q, const void* kv, void* out, int n_seq, int Lq, int Lk, int heads, int dim_head,
                            int64_t q_seq_stride, int64_t q_row_stride, int64_t kv_seq_stride, int64_t kv_row_stride, int64_t o_seq_stride,
                            int64_t o_row_stride, float scale);
/* VR networks, half-precision mode (csrc/vrnet_h.h): channels-last IEEE half tensors.
 * alsep_vr_conv2d on the f16 matrix pipe: x [B, H, W, Cin] half, w [Cout][Kp] half with k = (dy, dx, ci) zero-padded from KH KW Cin to Kp (a
 * multiple of 32), y [B, Ho, Wo, y_ctotal] at channel y_coff = act(conv * scale + shift), half (y_f16) or float32; act 0 / 1 ReLU / 2 LeakyReLU */
int alsep_vr_conv_h(alsep_ctx* ctx, const void* x, const void* w, const float* scale, const float* shift, void* y, int y_f16, int64_t B, int H,
                    int W, int Cin, int Cout, int Kp, int KH, int KW, int stride, int pad_h, int pad_w, int dil_h, int dil_w, int act,
                    int y_ctotal, int y_coff);
/* The decoder's convolution without its concatenated input: channels [0, Cu) are x [B, Hu, Wu, Cu] resized x2 (bilinear, align_corners;
 * float32 arithmetic, rounded to half: the bits of alsep_vr_resize_bilinear_h), channels [Cu, Cu + Cs) are skip [B, 2 Hu, Ws, Cs] at columns
 * w_off .. w_off + 2 Wu - 1.  KH x KW, stride 1, padding pad; everything else as alsep_vr_conv_h. */
int alsep_vr_decoder_conv_h(alsep_ctx* ctx, const void* x, const void* skip, const void* w, const float* scale, const float* shift, void* y,
                            int y_f16, int64_t B, int Hu, int Wu, int Cu, int Ws, int Cs, int w_off, int Cout, int Kp, int KH, int KW, int pad,
                            int act, int y_ctotal, int y_coff);
/* alsep_vr_depthwise / _resize_bilinear / _copy_slice / _mean_h on half tensors (depthwise weights half; float32 arithmetic) */
int alsep_vr_depthwise_h(alsep_ctx* ctx, const void* x, const void* w, void* y, int64_t B, int H, int W, int C, int KH, int KW, int pad, int dil);
int alsep_vr_resize_bilinear_h(alsep_ctx* ctx, const void* x, void* y, int64_t B, int H, int W, int C, int Ho, int Wo, int y_ctotal, int y_coff);
int alsep_vr_copy_slice_h(alsep_ctx* ctx, const void* x, void* y, int64_t BH, int Wx, int C, int w_off, int Wy, int y_ctotal, int y_coff);
int alsep_vr_mean_hh(alsep_ctx* ctx, const void* x, void* y, int64_t B, int H, int W, int C);
/* Roformer band split, input side, all bands in one launch: feat[band][t][kmax] (half) = RMSNorm over the band's `width[band]` gathered
 * spectrogram values of frame t (spec [4][F][T]; pidx[band][kmax / 2] merged bin index 2 f + s or -1; gamma[band][kmax]), zero-padded */
int alsep_roformer_bandsplit_in(alsep_ctx* ctx, const float* spec, const int* pidx, const float* gamma, const int* width, void* feat, int nb,
                                int F, int T, int kmax);
/* table[pos][j] = (cos, sin)(pos / 10000^(2 j / dim_head)), pos < L, j < dim_head / 2 (rotary_embedding_torch, interleaved pairs) */
int alsep_nn_rotary_table(alsep_ctx* ctx, float* table, int L, int dim_head);

/* ---- reverb impulse-response extraction: replaces handlers/reverb.py:112-172 (extract_reverb), called from
 * modules/separator/stem_separator.py:822-829 when a de-reverb transform ran on the vocals with store_reverb_ir.  Whole-track FFT work in
 * double precision (csrc/reverb.hip).  Audio arguments: float32 device tensors [channels][n] with row stride ld; the mono signals are
 * np.mean over the channels as reverb.py:52-53.  All functions need a workspace of alsep_reverb_workspace_bytes(n_wet, n_dry) bytes
 * (-1: a signal is too long, > 2^27 transform points). */
int64_t alsep_reverb_workspace_bytes(int64_t n_wet, int64_t n_dry);
/* fft_xcorr (reverb.py:55-66) + np.argmax over its n_wet + n_dry - 1 entries (:130-131) -> *argmax_out (host).  Optionally the
 * correlation values at probe_idx[0 .. n_probe) (host indices) -> probe_out (host), for tests.  Synchronises the stream. */
int alsep_reverb_xcorr_argmax(alsep_ctx* ctx, const float* wet, int c_wet, int64_t n_wet, int64_t ld_wet, const float* dry, int c_dry,
                              int64_t n_dry, int64_t ld_dry, void* ws, int64_t ws_bytes, int64_t* argmax_out, double* probe_out,
                              const int64_t* probe_idx, int n_probe);
/* wiener_deconvolution(wet_mono, dry_mono, eps)[:n_out] (reverb.py:94-106, :142-143) -> ir_out (device, float64); the deconvolution has
 * 2 * (n_wet / 2) samples (np.fft.irfft's default length), *n_written (host) = min(n_out, that). */
int alsep_reverb_wiener_ir(alsep_ctx* ctx, const float* wet, int c_wet, int64_t n_wet, int64_t ld_wet, const float* dry, int c_dry,
                           int64_t n_dry, int64_t ld_dry, double eps, void* ws, int64_t ws_bytes, double* ir_out, int64_t n_out,
                           int64_t* n_written);
/* the curve estimate_rt60 fits (reverb.py:74-81), in its float32 arithmetic: 20 log10(sqrt(sum_c x^2) + 1e-10) -> out [n] (device) */
int alsep_reverb_envelope_db(alsep_ctx* ctx, const float* x, int c, int64_t n, int64_t ld, float* out);
/* |np.fft.rfft(x)| of a real float64 device signal of any length n (spectral centroid, reverb.py:155-157) -> mag_out [n / 2 + 1];
 * workspace: (2 n) * 16 + alsep_dft_f64_workspace_bytes(n) bytes */
int alsep_rfft_mag_f64(alsep_ctx* ctx, const double* x, int64_t n, void* ws, int64_t ws_bytes, double* mag_out);
/* complex DFT of any length n <= 2^27 on interleaved float64 (re, im) device data, unnormalised (inverse != 0: the conjugate kernel);
 * in != out; workspace alsep_dft_f64_workspace_bytes(n) */
int64_t alsep_dft_f64_workspace_bytes(int64_t n);
int alsep_dft_f64(alsep_ctx* ctx, const double* in, double* out, int64_t n, int inverse, void* ws, int64_t ws_bytes);

/* ---- convolution reverb: replaces apply_reverb of handlers/reverb.py:179-209 (called from wrappers/merge.py:118 with the
 * impulse_response.ir file that extract_reverb stored).  out[c] = clip(dry[c] + wet_gain * wet[c], -1, 1) with
 * wet[c] = np.pad(fftconvolve(dry[c], ir, "full"), (pre_delay_samples, 0))[:n], float32 [channels][n] tensors with row strides ld /
 * ld_out, ir: n_ir float64 taps on the device (1 .. 2^20).  Overlap-save in double precision on blocks of F = 2^k >= 2 n_ir points
 * (log2_block = k, or 0: max(ceil(log2(2 n_ir)), 10)), two channels per complex transform.  The workspace holds the IR's spectrum and two
 * F-point buffers per block of a batch: ws_bytes decides how many blocks run side by side (at least one), the result does not depend on
 * it.  out must not overlap dry.  ALSEP_ERR_ARG: n_ir above the cap, a block too short for it, a negative pre-delay. */
int alsep_reverb_apply_block_log2(int64_t n_ir, int log2_block);              /* k, or -1 for a bad geometry */
int64_t alsep_reverb_apply_workspace_bytes(int64_t n_ir, int log2_block, int blocks_per_batch);   /* -1 for a bad geometry */
int alsep_reverb_apply(alsep_ctx* ctx, const float* dry, int channels, int64_t n, int64_t ld, const double* ir, int64_t n_ir,
                       int64_t pre_delay_samples, double wet_gain, int log2_block, float* out, int64_t ld_out, void* ws, int64_t ws_bytes);

/* ---- pitch shifting of a stem by `ratio` = 2^(semitones / 12), 1/4 <= ratio <= 4: the "transpose the song" step of wrappers/merge.py:125-127
 * (util/audio_track.py:603-694 shells out to ffmpeg's rubberband filter there; this is the project's own shifter, parity unpinned).  A phase
 * vocoder with identity phase locking (n_fft a power of two, 256 .. 8192, synthesis hop n_fft / 4, analysis hop n_fft / (4 ratio), periodic
 * Hann) stretches x by `ratio`, a Kaiser-windowed sinc (64 zero crossings, beta 14.7697, roll-off 0.9476) resamples the result back to n
 * samples; DESIGN section 4c has the arithmetic.  float32 [channels][n] tensors with row strides ld / ld_out, channels independent; double
 * precision on the device, one rounding to float32.  Frames travel in batches of frames_per_batch >= 4: the workspace depends on the batch,
 * not on n, and the result does not depend on the batch by a bit.  out must not overlap x. */
int64_t alsep_pitch_shift_frames(int64_t n, int n_fft, double ratio);         /* analysis frames U = ceil(n ratio / (n_fft / 4)) + 1; -1: bad geometry */
int64_t alsep_pitch_shift_workspace_bytes(int channels, int n_fft, int frames_per_batch, double ratio);   /* -1 for a bad geometry */
int alsep_pitch_shift(alsep_ctx* ctx, const float* x, int channels, int64_t n, int64_t ld, double ratio, int n_fft, int frames_per_batch,
                      float* out, int64_t ld_out, void* ws, int64_t ws_bytes);

/* ---- the arithmetic of the Compare plugin (wrappers/compare.py:92-124, :145, :152): two float64 tracks of n >= 2048 samples at the common
 * rate, RMS-normalised, their absolute difference, and scipy.signal.stft(x, nperseg=2048, noverlap=1024) of both -- periodic Hann, zero
 * boundary, padded tail, scaled by 1 / sum(window): F = 1 + ceil(n / 1024) frames, frame f holding the samples [1024 f - 1024, 1024 f + 1024)
 * -- as 20 log10(S1 + 1e-9) and 20 log10(|S1 - S2| + 1e-9).  Float64 on the device; the decibel arrays are float32 [1025][F].  n <= 2^31. */
int64_t alsep_compare_frames(int64_t n);                                      /* F, or -1 for n < 2048 or n > 2^31 */
/* *sumsq_out (device) = the sum of the squares of x[0 .. n) in a reduction order that depends on n alone: the same bits on every run, no
 * floating-point atomics.  ws: alsep_compare_rms_workspace_bytes() bytes. */
int64_t alsep_compare_rms_workspace_bytes(void);
int alsep_compare_rms(alsep_ctx* ctx, const double* x, int64_t n, double* sumsq_out, void* ws, int64_t ws_bytes);
/* sumsq: device, [2], the sums of squares of x0 and x1 over n samples.  w_i = x_i / rms_i where rms_i = sqrt(sumsq[i] / n) > 1e-9, else
 * x_i as it is (:96-99); diff = |w0 - w1| (:102).  The outputs overlap nothing. */
int alsep_compare_wave(alsep_ctx* ctx, const double* x0, const double* x1, int64_t n, const double* sumsq, double* w0, double* w1, double* diff);
/* window: device, float64 [2048], the periodic Hann window; twiddle: device, interleaved float64 (re, im) [2048], exp(-2 pi i m / 2048);
 * both computed by the caller on the host.  The two frames of a column go through one 2048-point complex transform in LDS, one workgroup
 * per frame, at most frames_per_batch frames per launch (0: the default, 65536); the result does not depend on it.  spec1_db, diff_db:
 * float32 [1025][F]; s1_lin, sd_lin: S1 and |S1 - S2| themselves, float64 [1025][F], or NULL. */
int alsep_compare_spectra(alsep_ctx* ctx, const double* w0, const double* w1, int64_t n, const double* window, const double* twiddle,
                          int frames_per_batch, float* spec1_db, float* diff_db, double* s1_lin, double* sd_lin);
/* Bucket j of `buckets` (1 .. n) holds the samples [floor(j n / buckets), floor((j + 1) n / buckets)): its smallest and largest value with
 * the first index of each.  All outputs on the device, [buckets]. */
int alsep_compare_minmax(alsep_ctx* ctx, const double* x, int64_t n, int64_t buckets, double* mn, int64_t* imn, double* mx, int64_t* imx);
/* in: float32 [1025][frames]; out [1025][buckets] = the largest value of each bin over the frame buckets (same rule, 1 <= buckets <= frames) */
int alsep_compare_colmax(alsep_ctx* ctx, const float* in, int64_t frames, int64_t buckets, float* out);

/* ---- reference-track mastering: the arithmetic behind the Remaster plugin (wrappers/remaster.py:67-76 hands both files to the Matchering
 * library; this is the project's restatement of that published design, parity unpinned: tests/remaster_oracle.py).
 * Float64 on the device throughout; stereo signals are [2][n] rows with a row stride.  Each step is its own entry point; the host
 * (audiolab_amd/master.py) chains them and designs the matching FIR from the two averaged spectra.  n <= 2^30.  Reductions have a fixed
 * order (no floating-point atomics).  ws of the functions without a size function of their own: alsep_master_workspace_bytes(). */
int64_t alsep_master_workspace_bytes(void);
/* ms[0] = (L / divisor + R / divisor) / 2, ms[1] = (L / divisor - R / divisor) / 2 */
int alsep_master_midside(alsep_ctx* ctx, const double* lr, int64_t n, int64_t ld, double divisor, double* ms, int64_t ld_ms);
/* lr[0] = scale mid + scale side, lr[1] = scale mid - scale side */
int alsep_master_leftright(alsep_ctx* ctx, const double* ms, int64_t n, int64_t ld_ms, double scale, double* lr, int64_t ld);
/* sums[j] (device, j < d <= 64) = the sum of the squares of x[j p .. (j + 1) p), or of clip(scale x, -1, 1) when clip != 0; d p <= n */
int alsep_master_piece_sumsq(alsep_ctx* ctx, const double* x, int64_t n, int d, int64_t p, double scale, int clip, double* sums, void* ws,
                             int64_t ws_bytes);
/* *peak (device) = max|x| over rows (1 or 2) of n samples */
int alsep_master_peak(alsep_ctx* ctx, const double* x, int rows, int64_t n, int64_t ld, double* peak, void* ws, int64_t ws_bytes);
/* out[0][k], out[1][k], k <= n_fft / 2 (device): the mean of |rfft(frame)| scale / n_fft over the whole n_fft-sample frames of the listed
 * pieces (HOST array of n_pieces <= 64 piece indices; piece j = samples [j p, (j + 1) p)) of ms[0] and ms[1] -- scipy.signal.stft(pieces,
 * window="boxcar", nperseg=n_fft, noverlap=0, boundary=None, padded=False), magnitudes averaged.  n_fft: a power of two, 256 .. 8192, <= p;
 * twiddle: device, interleaved float64 (re, im) [n_fft], exp(-2 pi i m / n_fft), computed by the caller on the host; scale >= 0. */
int alsep_master_spectrum(alsep_ctx* ctx, const double* ms, int64_t n, int64_t ld_ms, int64_t p, const int32_t* pieces, int n_pieces, int n_fft,
                          double scale, const double* twiddle, double* out, void* ws, int64_t ws_bytes);
/* out[c] = scale * scipy.signal.fftconvolve(x[c], fir[c], "same"), c < channels: float64 rows, fir: device float64 [channels][n_fir].  The
 * overlap-save blocks of alsep_reverb_apply (same block exponent rule, same workspace rule: its size decides how many blocks run side by
 * side, the result does not depend on it); out must not overlap x. */
int64_t alsep_master_convolve_workspace_bytes(int64_t n_fir, int log2_block, int blocks_per_batch);
int alsep_master_convolve_same(alsep_ctx* ctx, const double* x, int channels, int64_t n, int64_t ld, const double* fir, int64_t n_fir, double scale,
                               int log2_block, double* out, int64_t ld_out, void* ws, int64_t ws_bytes);
/* centred != 0: out[i] = max x[i - (w - 1) .. i + (w - 1)], scipy.ndimage.maximum_filter1d(x, size=2 w - 1) with its "reflect" edges;
 * else out[i] = max x[max(0, i - w + 1) .. i].  2 w - 1 <= 8191; ALSEP_ERR_ARG for n < 2 w - 1.  out != x. */
int alsep_master_slide_max(alsep_ctx* ctx, const double* x, int64_t n, int w, int centred, double* out);
/* y = scipy.signal.lfilter([b0, b1], [1, a1], x, zi=[zi]) (reverse == 0), or the same filter run over x[::-1] with the result stored back
 * in x's order.  A scan: recurrences local to chunks of `chunk` samples (0: the default, 4096; at most 8192), a carry pass over the chunk
 * ends, a correction pass -- three launches.  |a1| <= 1; y != x. */
int64_t alsep_master_iir_workspace_bytes(int64_t n, int chunk);
int alsep_master_iir(alsep_ctx* ctx, const double* x, int64_t n, double b0, double b1, double a1, double zi, int reverse, int chunk, double* y,
                     void* ws, int64_t ws_bytes);
/* y = scipy.signal.filtfilt([b0, b1], [1, a1], x) with its defaults: odd extension by 6 samples (n >= 7), each pass started from zi times
 * the first sample it sees; zi = scipy.signal.lfilter_zi(b, a)[0], computed by the caller */
int64_t alsep_master_filtfilt_workspace_bytes(int64_t n, int chunk);
int alsep_master_filtfilt(alsep_ctx* ctx, const double* x, int64_t n, double b0, double b1, double a1, double zi, int chunk, double* y, void* ws,
                          int64_t ws_bytes);
/* the limiter's front: g = 1 - 1 / rect, rect = max(max(|L|, |R|), threshold) / threshold; *over (device) = 1 when some rect is not
 * numpy.isclose to 1 (|rect - 1| > 1e-8 + 1e-5), else 0 */
int alsep_master_rectify(alsep_ctx* ctx, const double* lr, int64_t n, int64_t ld, double threshold, double* g, int32_t* over);
int alsep_master_maximum(alsep_ctx* ctx, const double* a, const double* b, int64_t n, double* out);   /* out = max(a, b) */
/* the limiter's back: gain = 1 - max(s_h, g_a, max(h, rel)) (stored when gain != NULL), out = lr * gain, *peak (device) = max|out| */
int alsep_master_limit_apply(alsep_ctx* ctx, const double* lr, int64_t n, int64_t ld, const double* s_h, const double* g_a, const double* h,
                             const double* rel, double* out, int64_t ld_out, double* gain, double* peak, void* ws, int64_t ws_bytes);
/* result = lr / divisor (not lr itself); pcm (device, uint8 [6 n]): 24-bit PCM as libsndfile writes doubles -- rint(result 8388607), ties to
 * even, clipped to +/-8388607, little-endian 3-byte samples, L R interleaved */
int alsep_master_pcm24(alsep_ctx* ctx, const double* lr, int64_t n, int64_t ld, double divisor, double* result, int64_t ld_res, uint8_t* pcm);

/* ---- tempo and beat tracking: replaces librosa.load + librosa.beat.beat_track of wrappers/export.py:18-40 (csrc/tempo.h; parity unpinned,
 * specification tests/tempo_oracle.py).  Fixed geometry: 22050 Hz, n_fft 2048, hop 512, centred frames (F = 1 + n / 512), 128 mel bands,
 * tempogram window 344.  Float64 throughout; every pointer is a device pointer unless it says otherwise. */
/* F for n samples; -1 when n < 1 or n is more than 60 minutes */
int64_t alsep_tempo_frames(int64_t n);
/* mel [128][F] = filterbank . |rfft(frame window)|^2.  window: periodic Hann [2048]; twiddle: exp(-2 pi i m / 2048) as (re, im) pairs [2048];
 * bands: int32 [128][3] = first bin, bin count, offset into weights [n_weights] */
int alsep_tempo_mel(alsep_ctx* ctx, const double* y, int64_t n, const double* window, const double* twiddle, const int32_t* bands,
                    const double* weights, int64_t n_weights, double* mel);
/* db [128][frames] = max(D, max(D) - 80), D = 10 log10(max(1e-10, mel)); env [frames]: 3 zeros, then the median over the bands of
 * max(0, db[:, t] - db[:, t - 1]) for t = 1 .., cut to `frames` values */
int64_t alsep_tempo_flux_workspace_bytes(void);
int alsep_tempo_flux(alsep_ctx* ctx, const double* mel, int64_t frames, double* db, double* env, void* ws, int64_t ws_bytes);
/* stats [3] = max|env|, mean(env), std(env, ddof = 1) */
int alsep_tempo_env_stats(alsep_ctx* ctx, const double* env, int64_t frames, double* stats);
/* tg [344] = the mean over the frames of autocorrelate(window . frame) / max|.|, the frames 344 long, hop 1, over env padded by 172 with a
 * linear ramp to 0 on both sides.  window: periodic Hann [344] */
int64_t alsep_tempo_tempogram_workspace_bytes(void);
int alsep_tempo_tempogram(alsep_ctx* ctx, const double* env, int64_t frames, const double* window, double* tg, void* ws, int64_t ws_bytes);
/* ls = scipy.signal.convolve(env / stats[2], window, "same"); window [2 period + 1], 1 <= period <= 343 */
int alsep_tempo_local_score(alsep_ctx* ctx, const double* env, int64_t frames, const double* stats, const double* window, int period, double* ls);
/* Ellis' beat recursion over the offsets first_offset .. first_offset + count - 1 (all negative, at most 576 of them, first_offset >= -686):
 * cand[j] = txwt[j] + cum[i + offset j] (0 before the start); b = the lowest index among the maxima; cum[i] = ls[i] + cand[b];
 * back[i] (int32) = -1 until a frame has ls[i] >= 0.01 max(ls), i + offset b from then on.  Additions and comparisons only. */
int alsep_tempo_beat_dp(alsep_ctx* ctx, const double* ls, int64_t frames, const double* txwt, int first_offset, int count, double* cum,
                        int32_t* back);

/* ---- stem mixdown with loudness matching: replaces the pydub calls of wrappers/merge.py:15-45,146-151 (AudioSegment.overlay,
 * effects.normalize, .dBFS, .apply_gain), i.e. audioop.add / max / rms / mul, on the signed integer grid of `bits` (16 or 32) with
 * full scale M = 2^(bits-1).  The mix is int32 [channels][n] (row stride ld) for both widths; channels * n <= 2^31.
 * 16-byte loads and stores are used on every operand whose rows start on 16-byte boundaries, scalar ones elsewhere. */
#define ALSEP_MIX_MAX_STEMS 8
typedef struct alsep_mix_stem {
    const float* data;     /* device, float32 [channels][n], row stride ld */
    int64_t n, ld;
    int32_t channels;      /* that of the mix, or 1: feeds every channel */
    int32_t bits;          /* source width b_s <= bits: the sample's grid value is q_{b_s}(x) << (bits - b_s),
                            * q_b(x) = clip(rint(x 2^(b-1)), -2^(b-1), 2^(b-1) - 1), ties to even, NaN -> 0 */
} alsep_mix_stem;
/* acc = prev (or 0), then for each stem in order acc = clip(acc + v_k, -M, M - 1) (audioop.add saturates after every add) over the
 * samples < min(n, n_k); *peak (device) = max|acc| of the result, |-M| = M included.  `stems` is a HOST array of n_stems <=
 * ALSEP_MIX_MAX_STEMS entries; longer lists are chained through prev (which may be acc itself): the result does not depend on
 * the split.  acc must not overlap a stem. */
int alsep_mix_sum(alsep_ctx* ctx, const int32_t* prev, int64_t ld_prev, const alsep_mix_stem* stems, int n_stems, int channels, int64_t n,
                  int bits, int32_t* acc, int64_t ld_acc, uint32_t* peak);
/* y1 = floor(clip(acc f1, -M, M - 1)) (audioop.mul), not written: out (device) [0] = max|y1|, [1] / [2] = the sums of the high / low
 * 32 bits of every y1^2, so that sum y1^2 = out[1] 2^32 + out[2] exactly.  Block partials in ws, finished by one block. */
int64_t alsep_mix_power_workspace_bytes(int channels, int64_t n);
int alsep_mix_power(alsep_ctx* ctx, const int32_t* acc, int channels, int64_t n, int64_t ld, int bits, double f1, void* ws, int64_t ws_bytes,
                    uint64_t* out);
/* out_i = floor(clip(y1 f2, -M, M - 1)) with y1 as above; out_f (optional, float32) = out_i / M.  out_i may be acc itself. */
int alsep_mix_finish(alsep_ctx* ctx, const int32_t* acc, int channels, int64_t n, int64_t ld, int bits, double f1, double f2, int32_t* out_i,
                     int64_t ld_i, float* out_f, int64_t ld_f);

/* ---- the sum pass for operands of differing sample rates: audioop.ratecv(data, width, channels, in_rate, out_rate, None) -- what
 * pydub's AudioSegment.overlay reaches through _sync / set_frame_rate -- inside the sum.  With weightA = 1, weightB = 0 and no state the
 * routine is linear interpolation on 32-bit values: both rates divided by their gcd give inr, outr (1 .. 2^20 each); for a sample u on
 * the grid of width w (16 or 32) let x = u << (32 - w); output k of N inputs, k < K = floor((N - 1) outr / inr) + 1, is
 *     j = ceil(k inr / outr), d = j outr - k inr, o = (int)(((double)x[j - 1] d + (double)x[j] (outr - d)) / outr), x[-1] = 0,
 * truncated toward zero, and the result is o >> (32 - w) (arithmetic).  Channels are independent. */
typedef struct alsep_mix_operand {
    const void* data;      /* device: float32 [channels][n] (a stem) or int32 [channels][n] (the running mix, is_mix != 0), row stride ld */
    int64_t n, ld;
    int64_t in_rate, out_rate;   /* both 0, or equal: the operand is added as it is; else it is resampled from in_rate to out_rate */
    int32_t channels;      /* that of the result, or 1 (stems only): feeds every channel */
    int32_t bits;          /* a stem: its source width b_s as in alsep_mix_stem, resampled on that grid: ratecv_{b_s}(q_{b_s}(x)) << (bits - b_s);
                            * the mix: the grid it is resampled on, ratecv_b(mix >> (bits - b)) << (bits - b) -- the width of the widest
                            * stem in it.  16 or 32 wherever a rate pair is given */
    int32_t is_mix;        /* only operand 0 may be the mix; without a rate pair it may be acc itself */
} alsep_mix_operand;
/* K above, n when the rates are equal; -1: n < 1 or > 2^31, a rate < 1, or a reduced rate above 2^20 */
int64_t alsep_mix_ratecv_length(int64_t n, int64_t in_rate, int64_t out_rate);
/* acc = 0, then for each operand in order acc = clip(acc + v_k, -M, M - 1) over the samples below min(n_out, the operand's length after
 * resampling); *peak (device) = max|acc| as alsep_mix_sum.  `operands` is a HOST array of 1 .. ALSEP_MIX_MAX_STEMS entries.  Operand 0
 * sets the length: n_out must equal its length after resampling.  A resampled operand must not overlap acc (a thread reads samples its
 * neighbours write).  ALSEP_ERR_ARG before any launch for anything else: a rate < 1 beside a rate, a reduced rate above 2^20, a width
 * other than 16 or 32 with a rate pair, channels * n_out > 2^31. */
int alsep_mix_sum_rates(alsep_ctx* ctx, const alsep_mix_operand* operands, int n_operands, int channels, int64_t n_out, int bits,
                        int32_t* acc, int64_t ld_acc, uint32_t* peak);

/* ---- RMVPE pitch extraction: replaces the RMVPE class of modules/rvc/infer/lib/rmvpe.py (csrc/rmvpe.h).  Float32, the decode in float64;
 * channels-last tensors; every pointer is a device pointer. ---- */
/* frames of n samples at 16 kHz: n / 160 + 1; -1 when n < 1 or the count is above 2^20 */
int64_t alsep_rmvpe_frames(int64_t n);
/* the log-mel front end (rmvpe.py:475-555, :113-149): the track reflected by 512 samples at both ends (folded as often as a short
 * track needs), frames of 1024 every 160, window [1024], the float32 magnitude of 513 bins, basis [128][513] . magnitude, and
 * mel_log [T][128] = log(max(., 1e-5)); mel_lin (may be NULL) [T][128]: the product before the clamp.  twiddle: exp(-2 pi i k / 1024) as
 * (re, im) pairs, k < 512; bands: int32 [128][2] = first bin and bin count of every row's non-zero stretch of the basis. */
int alsep_rmvpe_mel(alsep_ctx* ctx, const float* audio, int64_t n, const float* window, const float* twiddle, const float* basis,
                    const int32_t* bands, float* mel_lin, float* mel_log);
/* y [Tp][C] = scale * x[r(t)][C] + shift, r(t) = t below T and 2 (T - 1) - t from there on (mel2hidden's reflection of the frame axis,
 * rmvpe.py:608-622, with the input BatchNorm of the one channel folded in); ALSEP_ERR_ARG when Tp - T > T - 1 */
int alsep_rmvpe_pad_frames(alsep_ctx* ctx, const float* x, float* y, int64_t T, int64_t Tp, int C, float scale, float shift);
/* nn.AvgPool2d(2): x [B, H, W, C] -> y [B, H / 2, W / 2, C]; H and W even.  cat (may be NULL): x is also copied into the channel slice
 * [cat_coff, cat_coff + C) of cat [B, H, W, cat_ctotal] (the skip half of the decoder's torch.cat) */
int alsep_rmvpe_avgpool2(alsep_ctx* ctx, const float* x, float* y, int64_t B, int H, int W, int C, float* cat, int cat_ctotal, int cat_coff);
/* y[..., y_coff : y_coff + Cout] of [B, 2H, 2W, y_ctotal] = act(conv_transpose2d(x, w, stride 2, padding 1, output_padding 1) * scale +
 * shift); x [B, H, W, Cin]; w packed [3][3][Cin][Cout] from the module's [Cin][Cout][3][3]; act 0 or 1 (ReLU); Cout % 4 == 0 */
int alsep_rmvpe_tconv3x3s2(alsep_ctx* ctx, const float* x, const float* w, const float* scale, const float* shift, float* y, int64_t B, int H,
                           int W, int Cin, int Cout, int act, int y_ctotal, int y_coff);
/* One bidirectional GRU layer's recurrence (torch.nn.GRU, gate order r, z, n; n = tanh(pre_n + r (W_hn h + b_hn))), both directions and
 * all N sequences in ONE launch:
 *   pre [T, N, 6H] = x W_ih^T + b_ih of the forward (columns 0 .. 3H) and the reverse direction (3H .. 6H);
 *   whh_t [2, H, 3H] = W_hh^T and bhh [2, 3H] = b_hh of each direction (forward first);  h [T, N, 2H] = h_t, forward direction first.
 * Zero initial state.  16 <= H <= 512, H % 16 == 0. */
int alsep_nn_gru(alsep_ctx* ctx, const float* pre, const float* whh_t, const float* bhh, float* h, int T, int N, int H);
/* x = 1 / (1 + exp(-x)) in place */
int alsep_rmvpe_sigmoid(alsep_ctx* ctx, float* x, int64_t n);
/* to_local_average_cents + decode (rmvpe.py:624-628, :669-687): salience [T][360] float32 -> f0 [T] float64; 0 where the frame's largest
 * salience <= thred (compared in float32) and where f0 comes out as exactly 10 */
int alsep_rmvpe_decode(alsep_ctx* ctx, const float* salience, int64_t T, float thred, double* f0);

/* ---- RVC's NSF-HiFiGAN vocoder: replaces GeneratorNSF of modules/rvc/infer/lib/infer_pack/models.py (csrc/nsf.h).  Float32, the source's
 * phase in float64; channels-last [L, C]; every pointer is a device pointer; pointers that carry channels are 16-byte aligned.  The
 * contractions are exact f32 MFMA whatever alsep_nn_set_contraction says. ---- */
/* bytes of workspace alsep_nsf_source needs for T frames; -1 when T < 1 or T > 2^20 */
int64_t alsep_nsf_source_workspace_bytes(int64_t T);
/* SourceModuleHnNSF with no overtones (models.py:313-446): f0 [T] (0 where unvoiced), noise [T upp] standard-normal draws ->
 * har [T upp] = tanh(lin_w (0.1 sin(2 pi rad) uv + (uv ? 0.003 : 0.1 / 3) noise) + lin_b), uv = f0 > 0, rad = f0 / sr * j + acc[t] for
 * sample j = 1 .. upp of frame t, acc[t] = fmod(sum over s < t of step[s], 1), step = fmod(f0 / sr * upp + 0.5, 1) - 0.5 in float32 as
 * the reference computes it; the sum in float64, scanned in chunks of 1024 frames whatever the launch geometry.  upp 1 .. 1024. */
int alsep_nsf_source(alsep_ctx* ctx, const float* f0, int64_t T, int upp, int sr, const float* noise, float lin_w, float lin_b, float* har,
                     void* workspace, int64_t workspace_bytes);
/* y [L, Cout] = out_scale (acc + post(conv1d(lrelu(x, pre_slope), w, dilation, padding dilation (K - 1) / 2) + bias + res)): one
 * convolution of ResBlock1 (modules.py:223-236) with its residual, the running sum over the resblocks and their mean; conv_pre with
 * pre_slope 1.  x [L, Cin]; w packed [K][Cin][Cout]; bias [Cout], res and acc [L, Cout] may each be NULL (y may be res or acc, not x);
 * post 0 none, 1 tanh.  K odd 1 .. 11, dilation 1 .. 5, Cin and Cout multiples of 8 (16 for the unmasked kernels). */
int alsep_nsf_conv1d(alsep_ctx* ctx, const float* x, const float* w, const float* bias, const float* res, const float* acc, float* y, int64_t L,
                     int Cin, int Cout, int K, int dilation, float pre_slope, int post, float out_scale);
/* y [L] = tanh(conv1d(lrelu(x, 0.01), w [7][C], padding 3)): conv_post (models.py:562-564); x [L, C], C a multiple of 8 */
int alsep_nsf_conv_post(alsep_ctx* ctx, const float* x, const float* w, float* y, int64_t L, int C);
/* one upsampling stage with its source injection (models.py:546-549): y [L u, Cout] = conv_transpose1d(lrelu(x, 0.1), w, stride u,
 * padding (K - u) / 2) + bias + noise_conv(har); x [L, Cin]; w packed [K][Cin][Cout] from the module's [Cin][Cout][K]; har [L u s];
 * noise_conv = Conv1d(1, Cout, 2 s, stride s, padding s / 2) for s > 1 and Conv1d(1, Cout, 1) for s = 1, noise_w packed [2 s or 1][Cout].
 * ALSEP_ERR_ARG unless K - u is even and K >= u (otherwise the output is not L u long), K <= 8 u (the kernel walks at most 8 taps per
 * output phase), s is 1 or even (an odd stride's noise convolution is one sample short), Cin and Cout are multiples of 8. */
int alsep_nsf_tconv1d(alsep_ctx* ctx, const float* x, const float* w, const float* bias, const float* har, const float* noise_w,
                      const float* noise_b, float* y, int64_t L, int Cin, int Cout, int K, int u, int s);

#ifdef __cplusplus
}
#endif
#endif /* ALSEP_H */
