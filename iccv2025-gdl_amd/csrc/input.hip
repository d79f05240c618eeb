// input.hip -- the device-side stages of the reference's input pipeline.
//
// 1. log-magnitude STFT of a clipped waveform, what every dataset of the reference computes per sample on the host:
//        resamples[resamples > 1.] = 1.; resamples[resamples < -1.] = -1.
//        spectrogram = librosa.stft(resamples, n_fft=512, hop_length=353)      (256 / 128 for Kinetics-Sounds, VGGSound)
//        spectrogram = np.log(np.abs(spectrogram) + 1e-7)
//    (/root/reference/dataset/CramedDataset.py:62-66, KSDataset.py:144-149, VGGSoundDataset.py:117-122).
//    librosa is a third-party dependency that is not vendored in the reference; its published algorithm (librosa.stft,
//    defaults win_length = n_fft, window = 'hann' (periodic: scipy.signal.get_window(..., fftbins=True)), center = True)
//    is: pad the signal by n_fft/2 on both sides (pad_mode 'constant' = zeros since librosa 0.10, 'reflect' before),
//    frame t = padded[t*hop .. t*hop + n_fft), X[k][t] = sum_n frame[n] * hann[n] * exp(-2 pi i k n / n_fft),
//    k = 0 .. n_fft/2, 1 + L/hop frames.  Output [B][n_fft/2+1][frames] float32, the tensor the DataLoader yields.
//
//    One block = 4 frames of one waveform, one thread per frequency bin: a direct DFT in fp32 against an exact
//    (double-precision-generated) twiddle table in LDS.  12 032 frames x 257 bins x 512 samples is 3.2 GMAC for a
//    B=64 CREMA-D batch -- microseconds of VALU time, so an FFT would buy nothing and the direct sum is the more
//    accurate of the two in fp32.
//    gdl_wave_logspec is the same transform with the datasets' waveform staging in front of it, in the same launch: the PCM
//    decode scale, the mono mix-down, the tiling and the (random) window of librosa.load + np.tile + slicing
//    (KSDataset.py:139-144 and the same lines of the other datasets), and np.resize behind it where a dataset has one.  The
//    two kernels share ls_block(); they differ in where a sample of the window comes from and in the store.
//
// 2. ToTensor() + Normalize(mean, std) of decoded frames (CramedDataset.py:77-81): uint8 HWC -> float32 CHW,
//    ((x / 255) - mean[c]) / std[c] in that order of fp32 operations (bit-identical to torchvision on the CPU).
//
// 3. RandomResizedCrop(size) + RandomHorizontalFlip() + ToTensor() + Normalize() for training, Resize((size, size)) + ToTensor()
//    + Normalize() for evaluation (CramedDataset.py:76-88 and the same lines of the other datasets), one launch per batch:
//    every source frame has a descriptor (where it lies in one packed uint8 buffer, its size, the crop box, the flip flag), the
//    kernel crops, resizes with Pillow's antialiased bilinear filter, flips, normalises and writes float32 [B][3][T][h][w] --
//    the reference's torch.permute(images, (1, 0, 2, 3)) folded into the store.  The arithmetic is Pillow's ImagingResample
//    (what transforms.Resize calls on a PIL image), restated in tests/resize_ref.py: horizontal pass, then vertical, the
//    intermediate rounded to uint8, 22-bit integer coefficients made from double-precision triangle weights.  All of it on
//    pixels is int32, so the result equals the restatement bit for bit (tests/test_augment_gpu.py).
//    What stays on the host: decoding the files to PCM / uint8 frames, resampling the audio of the 22050 Hz datasets (CREMA-D,
//    AVE: librosa's resampler is a third-party filter design that is not restated here), and drawing the window starts, boxes and
//    flips (a few integers per sample, gdl/data.py).
#include "common.h"
#include "ops.h"

namespace gdl {

constexpr int LS_FPB = 4;  // frames per block

// Where the samples of a clip's fixed-length window come from.  at(p), 0 <= p < L, is the clipped sample p of the window.
// gdl_logspec: the host has staged the batch, [B][L] float32.
struct LsContiguous {
    const float* w;
    __device__ __forceinline__ float at(int p) const { return fminf(fmaxf(w[p], -1.f), 1.f); }
};
// gdl_wave_logspec: the decoded clip as the file stores it; sample p of the window is sample (start + p) mod len of the clip's
// periodic extension (s0 = start mod len), decoded (int16: x / 32768, exact in fp32) and mixed down ((l + r) / 2, which is
// np.mean over two channels in fp32).
struct LsClip {
    const unsigned char* clip;  // 4-byte aligned
    unsigned len, s0;           // len < 2^31, s0 < len
    int stereo, s16;
    __device__ __forceinline__ float at(int p) const {
        unsigned q = s0 + (unsigned)p;  // < 2^32
        if (q >= len) {
            q -= len;
            if (q >= len) q %= len;  // only a clip shorter than the window wraps more than once
        }
        float v;
        if (s16) {
            if (stereo) {
                const unsigned lr = ((const unsigned*)clip)[q];
                v = ((float)(short)(lr & 0xffffu) * (1.f / 32768.f) + (float)(short)(lr >> 16) * (1.f / 32768.f)) / 2.f;
            } else {
                v = (float)((const short*)clip)[q] * (1.f / 32768.f);
            }
        } else {
            const float* c = (const float*)clip;
            v = stereo ? (c[2 * (size_t)q] + c[2 * (size_t)q + 1]) / 2.f : c[q];
        }
        return fminf(fmaxf(v, -1.f), 1.f);
    }
};

// The transform of one block -- LS_FPB frames from f0 on, one thread per bin -- whatever the samples' source: twiddle table,
// windowed frames into LDS, direct DFT, log magnitude.  False for a thread without a bin; lm[j] is the value of frame f0 + j.
template <class Src>
__device__ __forceinline__ bool ls_block(const Src& src, int L, int n_fft, int hop, int frames, int reflect, int f0, float (&lm)[LS_FPB]) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ls_smem[];
    float2* tw = (float2*)ls_smem;               // [n_fft] (cos, sin)(2 pi n / n_fft)
    float* xw = (float*)(tw + n_fft);            // [LS_FPB][n_fft] windowed frames
    const int bins = n_fft / 2 + 1, pad = n_fft / 2;
    for (int n = threadIdx.x; n < n_fft; n += blockDim.x) {
        double s, c;
        sincospi(2.0 * (double)n / (double)n_fft, &s, &c);
        tw[n] = make_float2((float)c, (float)s);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < LS_FPB * n_fft; i += blockDim.x) {
        const int j = i / n_fft, n = i - j * n_fft;
        int p = (f0 + j) * hop + n - pad;  // index into the unpadded signal
        float v = 0.f;
        if (f0 + j < frames) {
            if (reflect) {  // numpy 'reflect': the edge sample is not repeated
                if (p < 0) p = -p;
                if (p >= L) p = 2 * (L - 1) - p;
            }
            if (p >= 0 && p < L) v = src.at(p);
        }
        const float hann = 0.5f - 0.5f * tw[n].x;  // periodic Hann
        xw[i] = v * hann;
    }
    __syncthreads();
    const int k = threadIdx.x;
    if (k >= bins) return false;
    float re[LS_FPB], im[LS_FPB];
#pragma unroll
    for (int j = 0; j < LS_FPB; ++j) re[j] = 0.f, im[j] = 0.f;
    const int msk = n_fft - 1;
    int idx = 0;  // (k * n) mod n_fft
#pragma unroll 4
    for (int n = 0; n < n_fft; ++n) {
        const float2 t = tw[idx];
#pragma unroll
        for (int j = 0; j < LS_FPB; ++j) {
            const float x = xw[j * n_fft + n];
            re[j] = fmaf(x, t.x, re[j]);
            im[j] = fmaf(-x, t.y, im[j]);
        }
        idx = (idx + k) & msk;
    }
#pragma unroll
    for (int j = 0; j < LS_FPB; ++j) lm[j] = logf(sqrtf(re[j] * re[j] + im[j] * im[j]) + 1e-7f);
    return true;
}

__global__ void logspec_kernel(const float* __restrict__ wave, float* __restrict__ out, int L, int n_fft, int hop, int frames,
                               int reflect) {
    const int b = blockIdx.y, f0 = blockIdx.x * LS_FPB, bins = n_fft / 2 + 1;
    float lm[LS_FPB];
    if (!ls_block(LsContiguous{wave + (size_t)b * L}, L, n_fft, hop, frames, reflect, f0, lm)) return;
    float* o = out + ((size_t)b * bins + threadIdx.x) * frames + f0;
#pragma unroll
    for (int j = 0; j < LS_FPB; ++j)
        if (f0 + j < frames) o[j] = lm[j];
}

int logspec_frames(int L, int hop) { return 1 + L / hop; }

int logspec(const float* wave, int B, int L, int n_fft, int hop, int reflect, float* out, hipStream_t st) {
    const int frames = logspec_frames(L, hop), bins = n_fft / 2 + 1;
    const int threads = (bins + 63) / 64 * 64;
    const size_t lds = (size_t)n_fft * sizeof(float2) + (size_t)LS_FPB * n_fft * sizeof(float);
    hipLaunchKernelGGL(logspec_kernel, dim3(ceil_div(frames, LS_FPB), B), dim3(threads), lds, st, wave, out, L, n_fft, hop, frames,
                       reflect);
    GDL_CHECK_LAUNCH("logspec_kernel");
    return GDL_OK;
}

// ---------------------------------------------------------------- waveform staging + log-magnitude STFT
// logspec_kernel's grid and LDS; only the frame loader differs (LsClip), and the store: element e = k * frames + t of the
// [bins][frames] spectrogram goes to every e + j * bins * frames < total of the sample's output, which is np.resize's flat
// re-layout (total = out_h * out_w; an element past it is dropped) and the plain store for total = bins * frames.  A block
// also writes its share of the staged window to wave_out when the caller wants it: samples [x * chunk, (x + 1) * chunk) for
// block x of the clip, so that every sample is written once whatever hop and n_fft are.
// A descriptor from a C caller may be anything: a sample whose clip does not lie inside the packed buffer, or whose window does
// not lie inside its tiled length, is written as NaN and nothing of it is read.
__global__ void wave_logspec_kernel(const unsigned char* __restrict__ src, long long src_bytes, const long long* __restrict__ desc,
                                    float* __restrict__ wave_out, float* __restrict__ out, int L, int n_fft, int hop, int frames,
                                    int reflect, long long total) {
    const int b = blockIdx.y, f0 = blockIdx.x * LS_FPB, bins = n_fft / 2 + 1;
    const long long* d = desc + (size_t)b * 6;
    const long long off = d[0], len = d[1], ch = d[2], fmt = d[3], start = d[4], limit = d[5];
    bool ok = off >= 0 && (off & 3) == 0 && off <= src_bytes && len >= 1 && len < (1ll << 31) && (ch == 1 || ch == 2) &&
              (fmt == GDL_WAVE_F32 || fmt == GDL_WAVE_S16) && start >= 0 && limit < (1ll << 31) && start <= limit - L;
    ok = ok && len * ch * (fmt == GDL_WAVE_S16 ? 2 : 4) <= src_bytes - off;  // (len * ch * 4 < 2^34)
    const long long plane = (long long)bins * frames;
    float* o = out + (size_t)b * (size_t)total;
    const int chunk = (int)(((long long)L + gridDim.x - 1) / gridDim.x);
    const long long w0l = (long long)blockIdx.x * chunk;
    const int w0 = w0l < L ? (int)w0l : L, w1 = L - w0 < chunk ? L : w0 + chunk;
    float* wo = wave_out ? wave_out + (size_t)b * L : nullptr;
    if (!ok) {
        if (threadIdx.x < bins)
            for (int j = 0; j < LS_FPB; ++j)
                if (f0 + j < frames)
                    for (long long i = (long long)threadIdx.x * frames + f0 + j; i < total; i += plane) o[i] = __builtin_nanf("");
        if (wo)
            for (int p = w0 + threadIdx.x; p < w1; p += blockDim.x) wo[p] = __builtin_nanf("");
        return;
    }
    const LsClip clip{src + off, (unsigned)len, (unsigned)(start % len), ch == 2, fmt == GDL_WAVE_S16};
    if (wo)
        for (int p = w0 + threadIdx.x; p < w1; p += blockDim.x) wo[p] = clip.at(p);
    float lm[LS_FPB];
    if (!ls_block(clip, L, n_fft, hop, frames, reflect, f0, lm)) return;
#pragma unroll
    for (int j = 0; j < LS_FPB; ++j)
        if (f0 + j < frames)
            for (long long i = (long long)threadIdx.x * frames + f0 + j; i < total; i += plane) o[i] = lm[j];
}

int wave_logspec(const void* src, size_t src_bytes, const long long* desc, int B, int L, int n_fft, int hop, int reflect, int out_h,
                 int out_w, float* wave_out, float* out, hipStream_t st) {
    const int frames = logspec_frames(L, hop), bins = n_fft / 2 + 1;
    const int threads = (bins + 63) / 64 * 64;
    const size_t lds = (size_t)n_fft * sizeof(float2) + (size_t)LS_FPB * n_fft * sizeof(float);
    const long long total = out_h ? (long long)out_h * out_w : (long long)bins * frames;
    hipLaunchKernelGGL(wave_logspec_kernel, dim3(ceil_div(frames, LS_FPB), B), dim3(threads), lds, st, (const unsigned char*)src,
                       (long long)src_bytes, desc, wave_out, out, L, n_fft, hop, frames, reflect, total);
    GDL_CHECK_LAUNCH("wave_logspec_kernel");
    return GDL_OK;
}

struct Norm3 {
    float mean[3], std[3];
};
__global__ __launch_bounds__(256) void frames_normalize_kernel(const unsigned char* __restrict__ in, float* __restrict__ out,
                                                              size_t n_img, int hw, Norm3 nm) {
    // one thread per pixel: 3 bytes in, one float into each of the 3 channel planes
    const size_t total = n_img * (size_t)hw;
    for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t n = i / hw, p = i - n * hw;
        const unsigned char* s = in + i * 3;
        float* o = out + n * 3 * (size_t)hw + p;
#pragma unroll
        for (int c = 0; c < 3; ++c) o[(size_t)c * hw] = ((float)s[c] / 255.f - nm.mean[c]) / nm.std[c];
    }
}

int frames_normalize(const unsigned char* in, size_t n_img, int H, int W, const float* mean, const float* std, float* out,
                     hipStream_t st) {
    Norm3 nm;
    for (int c = 0; c < 3; ++c) nm.mean[c] = mean[c], nm.std[c] = std[c];
    const size_t total = n_img * (size_t)H * W;
    const int grid = (int)((total + 255) / 256 > 16384 ? 16384 : (total + 255) / 256);
    hipLaunchKernelGGL(frames_normalize_kernel, dim3(grid), dim3(256), 0, st, in, out, n_img, H * W, nm);
    GDL_CHECK_LAUNCH("frames_normalize_kernel");
    return GDL_OK;
}

// ---------------------------------------------------------------- resized crop
// One block = RC_TILE output rows of one image, in four steps that never leave LDS:
//   tables    the 22-bit coefficients and tap bounds of the image's columns and of the block's rows, from the box and the output
//             size alone, in fp64 with Pillow's order of operations (no contraction: an fma would round differently); and the
//             normalise as a table over the 256 byte values (the two IEEE divisions per output were most of the vertical pass);
//   stage     the source rows the vertical taps of the rows need, only the box's columns, as dwords (a row starts at any byte:
//             the dwords that cover it are copied and the row's misalignment kept as an offset), as many rows at a time as fit,
//             RC_BATCH loads of a thread in flight;
//   horizontal  stage -> uint8 intermediate [source row][3][out column]: the taps' bytes are read as whole dwords and shifted
//             to byte 0 with v_alignbyte, so every byte sits at a fixed place (3, 5 and 7 taps unrolled; any other count loops);
//   vertical  intermediate -> flip -> normalise -> three channel planes: a thread owns four neighbouring columns of one channel
//             (the vertical coefficients do not depend on the column), so a tap is one dword LDS read and the result one
//             16-byte store; with the flip the four go out in reverse order at the mirrored place, still one contiguous store.
// How many source rows RC_TILE output rows need follows the vertical scale, so the block walks its rows in runs that fit the
// intermediate (a 1080-row box -> 224 takes 16 rows in several runs; an upscale in one).  LDS is carved per image by rc_plan();
// a box whose tables plus one staged row plus one output row's taps do not fit is refused (gdl_frames_resized_crop_box_ok on
// the host; from the kernel the image comes out as NaN, never as a wrong picture).
// The descriptors are device memory, so the host cannot size LDS to the boxes of a launch: it is a fixed 40 KB, which puts four
// blocks of 512 threads on a CU.  A block is a chain of short phases with barriers between them; what hides one block's HBM
// and LDS latencies is the other three.  The kernel is bound by VALU issue, not by HBM (profiles/augment_bench.txt): a
// multiply-add on a byte costs a byte extract and a 24-bit mad, and there are about ten of them per output value at 360 x 480 -> 224 x 224.
constexpr int RC_THREADS = 512;
constexpr int RC_TILE = 16;
constexpr int RC_LDS = 40 * 1024;  // four blocks a CU
constexpr int RC_MAX_DIM = 65535;  // source height / width
constexpr int RC_BITS = 22;        // Pillow's PRECISION_BITS for 8-bit pixels
constexpr int RC_LUT_BYTES = 3 * 256 * 4;  // ((v / 255) - mean[c]) / std[c] for the 256 values of a byte: two IEEE divisions per output otherwise

struct RcPlan {
    int ksx, ksy;         // taps per output column / row: 2 * ceil(max(1, in / out)) + 1
    int stride_dw;        // dwords per staged row (one more than the data can take: the two-dword reads look one ahead)
    int mrow;             // bytes per intermediate row: 3 planes of out_w rounded up to 4
    int stage_rows, mid_rows;
    int off_hb, off_vk, off_vb, off_stage, off_mid;  // byte offsets (the normalise table starts at 0, the column coefficients follow it)
};
__host__ __device__ inline int rc_ksize(int in, int out) { return 2 * (in > out ? (in + out - 1) / out : 1) + 1; }
__host__ __device__ inline bool rc_plan(int bh, int bw, int oh, int ow, RcPlan& p) {
    if (bh < 1 || bw < 1 || oh < 1 || ow < 1 || bh > RC_MAX_DIM || bw > RC_MAX_DIM || oh > RC_MAX_DIM || ow > RC_MAX_DIM) return false;
    p.ksx = rc_ksize(bw, ow);
    p.ksy = rc_ksize(bh, oh);
    p.stride_dw = (bw * 3 + 6) / 4 + 1;
    p.mrow = 3 * ((ow + 3) & ~3);
    const int pad = (3 * p.ksx + 11) & ~3;  // after the staged rows: taps with a zero coefficient past a row's end are read
    long long o = RC_LUT_BYTES + ((4ll * ow * p.ksx + 7) & ~7ll);  // (the bounds are int2: 8-byte aligned)
    p.off_hb = (int)o, o += 8ll * ow;
    p.off_vk = (int)o, o += (4ll * RC_TILE * p.ksy + 7) & ~7ll;
    p.off_vb = (int)o, o += 8ll * RC_TILE;
    const int srow = 4 * p.stride_dw, mrow = p.mrow;
    if (o + pad + srow + (long long)mrow * p.ksy > RC_LDS) return false;
    const int rest = RC_LDS - (int)o - pad;  // everything below fits 32 bits
    // the intermediate gets the rows a whole tile needs if it can have them, staging what is left (at least one row)
    int want = (RC_TILE * bh + oh - 1) / oh + p.ksy;
    want = want > bh ? bh : want;
    want = want < p.ksy ? p.ksy : want;
    const int most = (rest - srow) / mrow;  // >= ksy
    want = want > most ? most : want;
    int sr = (rest - want * mrow) / srow;   // >= 1
    p.stage_rows = sr > want ? want : sr;
    p.off_stage = (int)o;
    p.off_mid = p.off_stage + p.stage_rows * srow + pad;
    p.mid_rows = (RC_LDS - p.off_mid) / mrow;
    return p.mid_rows >= p.ksy;
}
int resized_crop_box_ok(int bh, int bw, int oh, int ow) {
    RcPlan p;
    return rc_plan(bh, bw, oh, ow, p) ? 1 : 0;
}

// Pillow's precompute_coeffs + normalize_coeffs_8bpc for output index i of a pass in -> out, bilinear filter (support 1)
__device__ void rc_coeffs(int in, int out, int ks, int i, int* __restrict__ k, int2* __restrict__ bound) {
#pragma clang fp contract(off)
    const double scale = (double)in / (double)out;
    const double filterscale = scale > 1.0 ? scale : 1.0;
    const double support = 1.0 * filterscale, ss = 1.0 / filterscale;
    const double center = ((double)i + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in) xmax = in;
    int n = xmax - xmin;
    if (n > ks) n = ks;  // (never: ks is Pillow's own bound on the taps)
    double ww = 0.0;
    for (int x = 0; x < n; ++x) {
        double w = ((double)(x + xmin) - center + 0.5) * ss;
        w = w < 0.0 ? -w : w;
        w = w < 1.0 ? 1.0 - w : 0.0;
        ww += w;
    }
    for (int x = 0; x < ks; ++x) {
        int c = 0;
        if (x < n) {
            double w = ((double)(x + xmin) - center + 0.5) * ss;
            w = w < 0.0 ? -w : w;
            w = w < 1.0 ? 1.0 - w : 0.0;
            if (ww != 0.0) w = w / ww;
            c = (int)(0.5 + w * (double)(1 << RC_BITS));
        }
        k[x] = c;
    }
    *bound = make_int2(xmin, n);
}

__device__ __forceinline__ int rc_clip8(int acc) {
    const int v = acc >> RC_BITS;
    return v < 0 ? 0 : v > 255 ? 255 : v;
}

constexpr int RC_BATCH = 8;  // global loads a thread has in flight while staging

// Horizontal pass over nr staged rows.  KS > 0: the tap count is a compile-time constant and the loop unrolls, so a thread's LDS
// reads are all requested before the first is used (the tables are zero-padded to ks taps; a tap past the row's end reads
// whatever follows and multiplies it by zero).  KS == 0: any tap count.
template <int KS>
__device__ __forceinline__ void rc_hpass(const unsigned int* __restrict__ stage, unsigned char* __restrict__ mid, const int* __restrict__ hk,
                                         const int2* __restrict__ hb, int ksx, int nr, int ow, float rcp_ow, int sdw, int mis0, int pmis,
                                         int mrow, int pw) {
    const int ks = KS ? KS : ksx;
    for (int i = threadIdx.x; i < nr * ow; i += RC_THREADS) {
        const int j = fdiv_small(i, ow, rcp_ow), xx = i - j * ow;
        const int* k = hk + xx * ks;
        const unsigned int* srow = stage + j * sdw;
        const int pos = ((mis0 + j * pmis) & 3) + hb[xx].x * 3;  // byte of the row's staged dwords where the first tap's pixel starts
        unsigned int a[3] = {1u << (RC_BITS - 1), 1u << (RC_BITS - 1), 1u << (RC_BITS - 1)};
        if constexpr (KS > 0) {
            // the 3 * KS bytes of the taps as whole dwords, shifted to start at byte 0: every byte then sits at a fixed place
            constexpr int ND = (3 * KS + 3) / 4;
            const unsigned int* wp = srow + (pos >> 2);
            unsigned int w[ND + 1], x[ND];
#pragma unroll
            for (int d = 0; d <= ND; ++d) w[d] = wp[d];
#pragma unroll
            for (int d = 0; d < ND; ++d) x[d] = __builtin_amdgcn_alignbyte(w[d + 1], w[d], pos & 3);
#pragma unroll
            for (int t = 0; t < KS; ++t) {
                const unsigned int kk = (unsigned int)k[t];  // < 2^23, pixel < 2^8: 24-bit multiplies are exact
#pragma unroll
                for (int c = 0; c < 3; ++c) a[c] += __umul24((x[(3 * t + c) >> 2] >> (8 * ((3 * t + c) & 3))) & 255u, kk);
            }
        } else {
            for (int t = 0; t < ks; ++t) {
                const int ps = pos + 3 * t;
                const unsigned int px = __builtin_amdgcn_alignbyte(srow[(ps >> 2) + 1], srow[ps >> 2], ps & 3);
                const unsigned int kk = (unsigned int)k[t];
                a[0] += __umul24(px & 255u, kk), a[1] += __umul24((px >> 8) & 255u, kk), a[2] += __umul24((px >> 16) & 255u, kk);
            }
        }
        unsigned char* m = mid + j * mrow + xx;
        m[0] = (unsigned char)rc_clip8((int)a[0]), m[pw] = (unsigned char)rc_clip8((int)a[1]), m[2 * pw] = (unsigned char)rc_clip8((int)a[2]);
    }
}

// Vertical pass over output rows [y0, y1) + flip + normalise + store.  mid: the intermediate from source row r0 on, rows < nrows.
template <int KS>
__device__ __forceinline__ void rc_vpass(const unsigned char* __restrict__ mid, const int* __restrict__ vk, const int2* __restrict__ vb,
                                         int ksy, int y0, int y1, int yb, int r0, int nrows, int ow, int mrow, int pw, bool flip, bool vec,
                                         const float* __restrict__ lut, float* __restrict__ o, size_t cs) {
    const int ks = KS ? KS : ksy, nq = pw >> 2;
    const float rcp_nq = 1.f / (float)nq;
    for (int i = threadIdx.x; i < (y1 - y0) * 3 * nq; i += RC_THREADS) {
        const int jc = fdiv_small(i, nq, rcp_nq), qd = i - jc * nq, j = jc / 3, c = jc - 3 * j, yy = y0 + j;
        const int* k = vk + (yy - yb) * ks;
        const int first = vb[yy - yb].x - r0;
        const unsigned int* m = (const unsigned int*)(mid + c * pw) + qd;
        unsigned int acc[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = 1u << (RC_BITS - 1);
#pragma unroll
        for (int t = 0; t < ks; ++t) {
            const int row = first + t < nrows ? first + t : nrows - 1;  // (a zero-coefficient tap past the run reads its last row)
            const unsigned int px = m[row * (mrow >> 2)], kk = (unsigned int)k[t];
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] += __umul24((px >> (8 * e)) & 255u, kk);
        }
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = lut[c * 256 + rc_clip8((int)acc[e])];
        float* q = o + c * cs + (size_t)yy * ow;
        const int x0 = 4 * qd;
        if (vec) {
            if (flip)
                *(float4*)(q + ow - 4 - x0) = make_float4(v[3], v[2], v[1], v[0]);
            else
                *(float4*)(q + x0) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (x0 + e < ow) q[flip ? ow - 1 - x0 - e : x0 + e] = v[e];
        }
    }
}

__global__ __launch_bounds__(RC_THREADS, 8) void resized_crop_kernel(const unsigned char* __restrict__ src, long long src_bytes,
                                                                  const long long* __restrict__ desc, int T, int oh, int ow,
                                                                  int tiles, Norm3 nm, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rc_smem[];
    const int tid = threadIdx.x;
    const int n = blockIdx.x / tiles, yb = (blockIdx.x - n * tiles) * RC_TILE;
    const int ye = yb + RC_TILE < oh ? yb + RC_TILE : oh;
    const long long* d = desc + (size_t)n * 8;
    const long long off = d[0], H = d[1], W = d[2];
    const bool flip = d[7] != 0;
    const size_t plane = (size_t)oh * ow, cs = (size_t)T * plane;  // channel stride of [B][3][T][oh][ow]
    float* o = out + ((size_t)(n / T) * 3 * T + (size_t)(n % T)) * plane;

    // a descriptor from a C caller may be anything: the frame must lie inside the packed buffer, the box is clamped into the frame
    bool ok = off >= 0 && H >= 1 && W >= 1 && H <= RC_MAX_DIM && W <= RC_MAX_DIM && off <= src_bytes && H * W * 3 <= src_bytes - off;
    int top = 0, left = 0, bh = 1, bw = 1;
    RcPlan p;
    if (ok) {
        const long long t0 = d[3] < 0 ? 0 : d[3] > H - 1 ? H - 1 : d[3], l0 = d[4] < 0 ? 0 : d[4] > W - 1 ? W - 1 : d[4];
        top = (int)t0, left = (int)l0;
        bh = (int)(d[5] < 1 ? 1 : d[5] > H - t0 ? H - t0 : d[5]);
        bw = (int)(d[6] < 1 ? 1 : d[6] > W - l0 ? W - l0 : d[6]);
        ok = rc_plan(bh, bw, oh, ow, p);
    }
    if (!ok) {
        for (int i = tid; i < (ye - yb) * ow; i += RC_THREADS)
            for (int c = 0; c < 3; ++c) o[c * cs + (size_t)yb * ow + i] = __builtin_nanf("");
        return;
    }
    float* lut = (float*)rc_smem;
    int* hk = (int*)(rc_smem + RC_LUT_BYTES);
    int2* hb = (int2*)(rc_smem + p.off_hb);
    int* vk = (int*)(rc_smem + p.off_vk);
    int2* vb = (int2*)(rc_smem + p.off_vb);
    unsigned int* stage = (unsigned int*)(rc_smem + p.off_stage);
    unsigned char* mid = rc_smem + p.off_mid;

    for (int i = tid; i < 3 * 256; i += RC_THREADS) {  // the expression of frames_normalize_kernel, once per byte value
        const int c = i >> 8;
        lut[i] = ((float)(i & 255) / 255.f - (c == 0 ? nm.mean[0] : c == 1 ? nm.mean[1] : nm.mean[2])) /
                 (c == 0 ? nm.std[0] : c == 1 ? nm.std[1] : nm.std[2]);
    }
    for (int i = tid; i < ow + (ye - yb); i += RC_THREADS) {
        if (i < ow)
            rc_coeffs(bw, ow, p.ksx, i, hk + i * p.ksx, hb + i);
        else
            rc_coeffs(bh, oh, p.ksy, yb + i - ow, vk + (i - ow) * p.ksy, vb + (i - ow));
    }
    __syncthreads();

    const long long pitch = W * 3;
    const int rowb = bw * 3, mrow = p.mrow, pw = mrow / 3, sdw = p.stride_dw, pmis = (int)(pitch & 3);
    const float rcp_ow = 1.f / (float)ow, rcp_sdw = 1.f / (float)sdw;
    const bool vec = pw == ow && ((size_t)out & 15) == 0;  // whole 16-byte stores
    for (int y0 = yb; y0 < ye;) {
        // the run of output rows [y0, y1) whose source rows [r0, r1) fit the intermediate (one row always does: rc_plan)
        const int r0 = vb[y0 - yb].x;
        int r1 = r0 + vb[y0 - yb].y, y1 = y0 + 1;
        while (y1 < ye && vb[y1 - yb].x + vb[y1 - yb].y - r0 <= p.mid_rows) {
            r1 = vb[y1 - yb].x + vb[y1 - yb].y;
            ++y1;
        }
        for (int c0 = r0; c0 < r1; c0 += p.stage_rows) {
            const int nr = r1 - c0 < p.stage_rows ? r1 - c0 : p.stage_rows, total = nr * sdw;
            // stage: the dwords that cover the box's bytes of rows c0 .. c0 + nr (src is 4-byte aligned: checked by the launcher),
            // RC_BATCH loads of a thread in flight at a time
            const long long a_first = off + (long long)(top + c0) * pitch + (long long)left * 3;
            const int mis0 = (int)(a_first & 3);
            for (int base = tid; base < total; base += RC_THREADS * RC_BATCH) {
                unsigned int v[RC_BATCH];
                long long a4[RC_BATCH];
#pragma unroll
                for (int u = 0; u < RC_BATCH; ++u) {
                    const int i = base + u * RC_THREADS, j = fdiv_small(i, sdw, rcp_sdw), q = i - j * sdw;
                    const long long a = a_first + (long long)j * pitch;
                    const int mis = (int)(a & 3);
                    a4[u] = i < total && q * 4 < mis + rowb ? a - mis + 4ll * q : -1;  // -1: nothing to load
                    v[u] = 0;
                    if (a4[u] >= 0 && a4[u] + 4 <= src_bytes) v[u] = *(const unsigned int*)(src + a4[u]);
                }
#pragma unroll
                for (int u = 0; u < RC_BATCH; ++u) {
                    if (a4[u] < 0) continue;
                    if (a4[u] + 4 > src_bytes)  // the last bytes of a buffer whose length is no multiple of 4
                        for (int e = 0; e < 4; ++e)
                            if (a4[u] + e < src_bytes) v[u] |= (unsigned int)src[a4[u] + e] << (8 * e);
                    stage[base + u * RC_THREADS] = v[u];
                }
            }
            __syncthreads();
            unsigned char* mrows = mid + (c0 - r0) * mrow;
            switch (p.ksx) {
                case 3: rc_hpass<3>(stage, mrows, hk, hb, 3, nr, ow, rcp_ow, sdw, mis0, pmis, mrow, pw); break;
                case 5: rc_hpass<5>(stage, mrows, hk, hb, 5, nr, ow, rcp_ow, sdw, mis0, pmis, mrow, pw); break;
                case 7: rc_hpass<7>(stage, mrows, hk, hb, 7, nr, ow, rcp_ow, sdw, mis0, pmis, mrow, pw); break;
                default: rc_hpass<0>(stage, mrows, hk, hb, p.ksx, nr, ow, rcp_ow, sdw, mis0, pmis, mrow, pw);
            }
            __syncthreads();
        }
        switch (p.ksy) {
            case 3: rc_vpass<3>(mid, vk, vb, 3, y0, y1, yb, r0, r1 - r0, ow, mrow, pw, flip, vec, lut, o, cs); break;
            case 5: rc_vpass<5>(mid, vk, vb, 5, y0, y1, yb, r0, r1 - r0, ow, mrow, pw, flip, vec, lut, o, cs); break;
            case 7: rc_vpass<7>(mid, vk, vb, 7, y0, y1, yb, r0, r1 - r0, ow, mrow, pw, flip, vec, lut, o, cs); break;
            default: rc_vpass<0>(mid, vk, vb, p.ksy, y0, y1, yb, r0, r1 - r0, ow, mrow, pw, flip, vec, lut, o, cs);
        }
        __syncthreads();  // the next run overwrites the intermediate
        y0 = y1;
    }
}

int frames_resized_crop(const unsigned char* src, size_t src_bytes, const long long* desc, int n_img, int T, int oh, int ow,
                        const float* mean, const float* std, float* out, hipStream_t st) {
    Norm3 nm;
    for (int c = 0; c < 3; ++c) nm.mean[c] = mean[c], nm.std[c] = std[c];
    const int tiles = ceil_div(oh, RC_TILE);
    hipLaunchKernelGGL(resized_crop_kernel, dim3((unsigned)n_img * tiles), dim3(RC_THREADS), RC_LDS, st, src, (long long)src_bytes,
                       desc, T, oh, ow, tiles, nm, out);
    GDL_CHECK_LAUNCH("resized_crop_kernel");
    return GDL_OK;
}

}  // namespace gdl
