// head_film.hip -- FiLM_DGL fusion head (/root/reference/models/fusion_modules.py:126-178), float32.
//
//   fc     : Linear(512*512, 512)   (134 M parameters: W[k][i*512 + j], the k-th row is a 512x512 matrix W_k)
//   fc_out : Linear(512, n)
//   output = fc_out(fc(flatten(x.detach() (x) y.detach())))     h_f[b][k] = x_b^T W_k y_b + bias_k
//   z_x    = fc_out(fc(flatten(x (x) x)))                       h_x[b][k] = x_b^T W_k x_b + bias_k
//   z_y    = fc_out(fc(flatten(y (x) y)))                       h_y[b][k] = y_b^T W_k y_b + bias_k
// The outer products are never materialised.  With fc.weight viewed as a [262144][512] row-major matrix
// A (row (k,i), column j) the heavy contractions are plain GEMMs over its 537 MB, and they run on the
// convolution kernels of this library in their exact-f32 mode (f32-input MFMA):
//   forward    T = A V^T,  V = [x; y] (2B rows)                      -> conv_fwd (1x1), T[(k,i)][b] = (W_k v_b)[i]
//              h_x[b][k] = sum_i x_b[i] T[(k,i)][b],  h_f / h_y from the y-columns of T
//   d x, d y   dx_b[i] = sum_k dh_x[b][k] ( (W_k x_b)[i] + (W_k^T x_b)[i] )
//              first term from T; second = U^T A with U[(k,j)][b] = dh_x[b][k] x_b[j]   -> conv_wgrad (1x1)
//   d fc.weight  dA = P Z^T, P[(k,i)][b] = dh[b][k] * (x|y)_b[i], Z = matching (y|x) rows -> conv_fwd (1x1)
// Everything else (V, U, P, the small contractions, fc_out and its gradients) is elementwise / tiny.
#include "common.h"
#include "gather.h"
#include "ops.h"

namespace gdl {

constexpr int FD = 512;            // feature width of both modalities and of fc's output
constexpr int FROWS = FD * FD;     // rows of fc.weight viewed as [FROWS][FD]

// the operand matrices have 2 Bp .. 3 Bp columns of FROWS rows (3 Bp: 1.6 GB at the limit), every index is size_t
constexpr int FILM_MAX_B = 512;
static inline int film_bp(int B) { return (B + 31) / 32 * 32; }  // batch padded so that 2*Bp % 64 == 0, 3*Bp % 32 == 0

// ---- V: planes of ld rows, plane 0 = x, plane 1 = y (rows 0..B-1 of a plane, padding rows zero), from plane p0 on: the DGL
// head's V[2*Bp][512] is (ld = Bp, p0 = 0, grid 2*Bp), the joint head's y rows alone (ld = Bj, p0 = 1, grid Bj)
__global__ void film_v_kernel(const float* __restrict__ x, const float* __restrict__ y, float* __restrict__ V, int B, int ld,
                              int p0) {
    const int r = blockIdx.x;
    const int b = r < ld ? r : r - ld;
    const float* src = b < B ? ((r < ld ? p0 : 1) ? y : x) + (size_t)b * FD : nullptr;
    for (int i = threadIdx.x; i < FD; i += blockDim.x) V[(size_t)r * FD + i] = src ? src[i] : 0.f;
}

// ---- h[b][k] = bias[k] + sum_i left_b[i] * T[(k,i)][col(b)]     grid = (512 k, forms, ceil(B / 64) sample groups):
// form = form0 + blockIdx.y: 0 = x form, 1 = fused, 2 = y form.  T has ld columns, W_k x_b at b, W_k y_b at ycol + b: the DGL
// head's three forms are (ld = 2*Bp, ycol = Bp, form0 = 0), the joint head's fused form alone (ld = Bj, ycol = 0, form0 = 1,
// one form; hx, hy unused) -- the same four slices of i and the same order of the partial sums
__global__ __launch_bounds__(256) void film_h_kernel(const float* __restrict__ T, const float* __restrict__ x,
                                                     const float* __restrict__ y, const float* __restrict__ bias,
                                                     float* __restrict__ hx, float* __restrict__ hf, float* __restrict__ hy,
                                                     int B, int ld, int ycol, int form0) {
    __shared__ float red[4][64];
    const int k = blockIdx.x, form = form0 + blockIdx.y;
    const float* left = form == 2 ? y : x;                 // x^T W_k x, x^T W_k y, y^T W_k y
    const int coff = form == 0 ? 0 : ycol;
    float* h = form == 0 ? hx : (form == 1 ? hf : hy);
    const int bl = threadIdx.x & 63, b = blockIdx.z * 64 + bl, part = threadIdx.x >> 6;  // 4 slices of i
    float s = 0.f;
    if (b < B) {
        const float* Tk = T + (size_t)k * FD * ld + coff + b;
        for (int i = part; i < FD; i += 4) s = fmaf(Tk[(size_t)i * ld], left[(size_t)b * FD + i], s);
    }
    red[part][bl] = s;
    __syncthreads();
    if (part == 0 && b < B) h[(size_t)b * FD + k] = ((red[0][bl] + red[1][bl]) + red[2][bl]) + red[3][bl] + bias[k];
}

// ---- logits of the three hidden vectors: grid = B.  Without UNI (the joint head) the fused set alone, from hf (hx, hy unused):
// the same products, lane order and butterfly
template <bool UNI>
__global__ __launch_bounds__(256) void film_out_kernel(const float* __restrict__ hx, const float* __restrict__ hf,
                                                       const float* __restrict__ hy, const float* __restrict__ Wo,
                                                       const float* __restrict__ bo, float* __restrict__ out,
                                                       float* __restrict__ x_out, float* __restrict__ y_out, int n) {
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float a[8], f[8], c[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        if (UNI) a[i] = hx[(size_t)b * FD + lane + 64 * i];
        f[i] = hf[(size_t)b * FD + lane + 64 * i];
        if (UNI) c[i] = hy[(size_t)b * FD + lane + 64 * i];
    }
    for (int j = wave; j < n; j += 4) {
        const float* w = Wo + (size_t)j * FD;
        float px = 0.f, pf = 0.f, py = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float wv = w[lane + 64 * i];
            if (UNI) px = fmaf(wv, a[i], px);
            pf = fmaf(wv, f[i], pf);
            if (UNI) py = fmaf(wv, c[i], py);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            if (UNI) px += __shfl_xor(px, o);
            pf += __shfl_xor(pf, o);
            if (UNI) py += __shfl_xor(py, o);
        }
        if (lane == 0) {
            out[(size_t)b * n + j] = pf + bo[j];
            if (UNI && x_out) x_out[(size_t)b * n + j] = px + bo[j];
            if (UNI && y_out) y_out[(size_t)b * n + j] = py + bo[j];
        }
    }
}

// ---- dh[form][b][k] = sum_c g_form[b][c] Wo[c][k]   (zero where the upstream gradient is absent)   grid = (B, 3)
__global__ __launch_bounds__(256) void film_dh_kernel(const float* __restrict__ g_x_out, const float* __restrict__ g_out,
                                                      const float* __restrict__ g_y_out, const float* __restrict__ Wo,
                                                      float* __restrict__ dh, int B, int n) {
    const int b = blockIdx.x, form = blockIdx.y;
    const float* g = form == 0 ? g_x_out : (form == 1 ? g_out : g_y_out);
    for (int k = threadIdx.x; k < FD; k += 256) {
        float s = 0.f;
        if (g)
            for (int c = 0; c < n; ++c) s = fmaf(g[(size_t)b * n + c], Wo[(size_t)c * FD + k], s);
        dh[((size_t)form * B + b) * FD + k] = s;
    }
}

// ---- dWo[c][k] = sum_b ( g_out h_f + uni (g_x_out h_x + g_y_out h_y) ), dbo likewise    grid = n
__global__ __launch_bounds__(256) void film_dwo_kernel(const float* __restrict__ hx, const float* __restrict__ hf,
                                                       const float* __restrict__ hy, const float* __restrict__ g_x_out,
                                                       const float* __restrict__ g_out, const float* __restrict__ g_y_out,
                                                       int uni, float* __restrict__ dWo, float* __restrict__ dbo, int B, int n) {
    const int c = blockIdx.x;
    for (int k = threadIdx.x; k < FD; k += 256) {
        float s = 0.f;
        for (int b = 0; b < B; ++b) {
            if (g_out) s = fmaf(g_out[(size_t)b * n + c], hf[(size_t)b * FD + k], s);
            if (uni) {
                if (g_x_out) s = fmaf(g_x_out[(size_t)b * n + c], hx[(size_t)b * FD + k], s);
                if (g_y_out) s = fmaf(g_y_out[(size_t)b * n + c], hy[(size_t)b * FD + k], s);
            }
        }
        dWo[(size_t)c * FD + k] = s;
    }
    if (threadIdx.x == 0) {
        float s = 0.f;
        for (int b = 0; b < B; ++b) {
            if (g_out) s += g_out[(size_t)b * n + c];
            if (uni) {
                if (g_x_out) s += g_x_out[(size_t)b * n + c];
                if (g_y_out) s += g_y_out[(size_t)b * n + c];
            }
        }
        dbo[c] = s;
    }
}

// ---- U[(k,j)][col], padding columns zero; one thread per (row, 4 columns).  XY (the DGL head): 2*Bp columns, col b ->
// dh_x[b][k] * x_b[j], col Bp+b -> dh_y[b][k] * y_b[j], the planes 0 / 2 of dh.  Without XY (the joint head): the one plane of Bp
// columns (the caller's Bj), col b -> dh[b][k] * x_b[j] with dh the fused plane; y unused.
template <bool XY>
__global__ __launch_bounds__(256) void film_u_kernel(const float* __restrict__ dh, const float* __restrict__ x,
                                                     const float* __restrict__ y, float* __restrict__ U, int B, int Bp) {
    const int cols = XY ? 2 * Bp : Bp, c4 = cols / 4;
    const size_t total = (size_t)FROWS * c4;
    for (size_t t = blockIdx.x * (size_t)256 + threadIdx.x; t < total; t += (size_t)gridDim.x * 256) {
        const int q = (int)(t % c4);
        const size_t row = t / c4;
        const int k = (int)(row / FD), j = (int)(row % FD);
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int col = q * 4 + e, isy = XY && col >= Bp, b = isy ? col - Bp : col;
            v[e] = b < B ? dh[((size_t)(isy ? 2 : 0) * B + b) * FD + k] * (isy ? y : x)[(size_t)b * FD + j] : 0.f;
        }
        *(float4*)(U + row * cols + q * 4) = make_float4(v[0], v[1], v[2], v[3]);
    }
}

// ---- dx[b][i] = out2[b][i] + sum_k dh_x[b][k] T[(k,i)][b];  dy from the y columns     grid = (B, 2)
__global__ __launch_bounds__(256) void film_dxy_kernel(const float* __restrict__ T, const float* __restrict__ dh,
                                                       const float* __restrict__ out2, float* __restrict__ dx,
                                                       float* __restrict__ dy, int B, int Bp) {
    const int b = blockIdx.x, isy = blockIdx.y;
    const float* dhb = dh + ((size_t)(isy ? 2 : 0) * B + b) * FD;
    const int col = (isy ? Bp : 0) + b;
    float* dst = (isy ? dy : dx) + (size_t)b * FD;
    for (int i = threadIdx.x; i < FD; i += 256) {
        float s = out2[(size_t)col * FD + i];
        for (int k = 0; k < FD; ++k) s = fmaf(dhb[k], T[((size_t)k * FD + i) * (2 * Bp) + col], s);
        dst[i] = s;
    }
}

// ---- operands of the fc.weight gradient GEMM: P[(k,i)][c], Z[j][c], c in blocks of Bp columns:
//   block 0: dh_f[b][k] * x_b[i]  with  Z = y_b[j];   (uni) block 1: dh_x[b][k] * x_b[i] with x_b[j];  block 2: dh_y[b][k] * y_b[i] with y_b[j]
__global__ __launch_bounds__(256) void film_p_kernel(const float* __restrict__ dh, const float* __restrict__ x,
                                                     const float* __restrict__ y, float* __restrict__ P, int B, int Bp,
                                                     int nblk) {
    const int cols = nblk * Bp, c4 = cols / 4;
    const size_t total = (size_t)FROWS * c4;
    for (size_t t = blockIdx.x * (size_t)256 + threadIdx.x; t < total; t += (size_t)gridDim.x * 256) {
        const int q = (int)(t % c4);
        const size_t row = t / c4;
        const int k = (int)(row / FD), i = (int)(row % FD);
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int col = q * 4 + e, blk = col / Bp, b = col - blk * Bp;
            const int form = blk == 0 ? 1 : (blk == 1 ? 0 : 2);  // dh index: 0 = x form, 1 = fused, 2 = y form
            v[e] = b < B ? dh[((size_t)form * B + b) * FD + k] * (blk == 2 ? y : x)[(size_t)b * FD + i] : 0.f;
        }
        *(float4*)(P + row * cols + q * 4) = make_float4(v[0], v[1], v[2], v[3]);
    }
}
__global__ void film_z_kernel(const float* __restrict__ x, const float* __restrict__ y, float* __restrict__ Z, int B, int Bp,
                              int nblk) {
    const int j = blockIdx.x, cols = nblk * Bp;  // Z[j][c]
    for (int c = threadIdx.x; c < cols; c += blockDim.x) {
        const int blk = c / Bp, b = c - blk * Bp;
        Z[(size_t)j * cols + c] = b < B ? (blk == 1 ? x : y)[(size_t)b * FD + j] : 0.f;
    }
}
// dbfc[k] = sum_b ( dh_f + uni (dh_x + dh_y) )
__global__ void film_dbfc_kernel(const float* __restrict__ dh, int uni, float* __restrict__ dbfc, int B) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= FD) return;
    float s = 0.f;
    for (int b = 0; b < B; ++b) {
        s += dh[((size_t)1 * B + b) * FD + k];
        if (uni) s += dh[((size_t)0 * B + b) * FD + k] + dh[((size_t)2 * B + b) * FD + k];
    }
    dbfc[k] = s;
}

// ---------------------------------------------------------------- workspace layout (bytes, 256-aligned pieces)
struct FilmWs {
    float *V, *T, *dh, *U, *out2, *P, *Z;
    void *tab_a, *tab_p, *wg;
    size_t wg_bytes, total;
};
// the head's contractions over fc.weight as plain GEMMs of the convolution kernels: FROWS rows, C -> K channels
static ConvGeom film_gemm(int C, int K) { return ConvGeom{1, FROWS, 1, C, K, 1, 1, 1, 0}; }
static FilmWs film_layout(unsigned char* base, int B) {
    const int Bp = film_bp(B);
    FilmWs w{};
    size_t off = 0;
    auto take = [&](size_t bytes) {
        void* p = base ? base + off : nullptr;
        off += (bytes + 255) / 256 * 256;
        return p;
    };
    w.V = (float*)take((size_t)2 * Bp * FD * 4);
    w.T = (float*)take((size_t)FROWS * 2 * Bp * 4);
    w.dh = (float*)take((size_t)3 * B * FD * 4);
    w.U = (float*)take((size_t)FROWS * 2 * Bp * 4);
    w.out2 = (float*)take((size_t)2 * Bp * FD * 4);
    w.P = (float*)take((size_t)FROWS * 3 * Bp * 4);
    w.Z = (float*)take((size_t)FD * 3 * Bp * 4);
    w.tab_a = take(gather_table_bytes(GATHER_FWD, film_gemm(FD, 2 * Bp)));  // (a table's size depends on the rows alone)
    w.tab_p = take(gather_table_bytes(GATHER_FWD, film_gemm(FD, 2 * Bp)));
    w.wg_bytes = conv_wgrad_ws_bytes(film_gemm(FD, 2 * Bp));
    w.wg = take(w.wg_bytes);
    w.total = off;
    return w;
}
size_t head_film_ws_bytes(int B) { return (B >= 1 && B <= FILM_MAX_B) ? film_layout(nullptr, B).total : 0; }

// hidden: [3][B][512] = h_x, h_f, h_y (kept by the caller for the backward, together with ws: T is reused)
int head_film_fwd(const float* x, const float* y, const float* Wfc, const float* bfc, const float* Wo, const float* bo,
                  float* hidden, float* out, float* x_out, float* y_out, int B, int n, void* ws, size_t ws_bytes, hipStream_t st) {
    GDL_REQUIRE(B >= 1 && B <= FILM_MAX_B, "head_film: B=%d (1..%d per call)", B, FILM_MAX_B);
    const FilmWs w = film_layout((unsigned char*)ws, B);
    if (!ws || ws_bytes < w.total) {
        set_error("head_film_fwd: workspace %zu < %zu bytes", ws_bytes, w.total);
        return GDL_ERR_WORKSPACE;
    }
    const int Bp = film_bp(B);
    float *hx = hidden, *hf = hidden + (size_t)B * FD, *hy = hidden + (size_t)2 * B * FD;
    hipLaunchKernelGGL(film_v_kernel, dim3(2 * Bp), dim3(256), 0, st, x, y, w.V, B, Bp, 0);
    GDL_CHECK_LAUNCH("film_v_kernel");
    int rc = build_gather_table(GATHER_FWD, GDL_F32, film_gemm(FD, 2 * Bp), (GatherEntry*)w.tab_a, st);
    if (rc) return rc;
    // T[(k,i)][col] = sum_j A[(k,i)][j] V[col][j]
    rc = conv_fwd(GDL_F32, Wfc, w.V, w.T, nullptr, w.tab_a, film_gemm(FD, 2 * Bp), st);
    if (rc) return rc;
    hipLaunchKernelGGL(film_h_kernel, dim3(FD, 3, (B + 63) / 64), dim3(256), 0, st, w.T, x, y, bfc, hx, hf, hy, B, 2 * Bp, Bp, 0);
    GDL_CHECK_LAUNCH("film_h_kernel");
    hipLaunchKernelGGL(film_out_kernel<true>, dim3(B), dim3(256), 0, st, hx, hf, hy, Wo, bo, out, x_out, y_out, n);
    GDL_CHECK_LAUNCH("film_out_kernel");
    return GDL_OK;
}

// Needs the workspace of the matching forward untouched (T).  Any upstream gradient may be NULL.
// dx/dy (pair), dWo/dbo (pair), dWfc/dbfc (pair) may be NULL.  uni: the unimodal logit sets also contribute to the
// parameter gradients (plain autograd); 0 in the DGL step (main_dgl.py:114-122 drops them).
int head_film_bwd(const float* x, const float* y, const float* Wfc, const float* Wo, const float* hidden,
                  const float* g_x_out, const float* g_y_out, const float* g_out, int uni, float* dx, float* dy, float* dWfc,
                  float* dbfc, float* dWo, float* dbo, int B, int n, void* ws, size_t ws_bytes, hipStream_t st) {
    GDL_REQUIRE(B >= 1 && B <= FILM_MAX_B, "head_film: B=%d (1..%d per call)", B, FILM_MAX_B);
    const FilmWs w = film_layout((unsigned char*)ws, B);
    if (!ws || ws_bytes < w.total) {
        set_error("head_film_bwd: workspace %zu < %zu bytes", ws_bytes, w.total);
        return GDL_ERR_WORKSPACE;
    }
    const int Bp = film_bp(B);
    const float *hx = hidden, *hf = hidden + (size_t)B * FD, *hy = hidden + (size_t)2 * B * FD;
    hipLaunchKernelGGL(film_dh_kernel, dim3(B, 3), dim3(256), 0, st, g_x_out, g_out, g_y_out, Wo, w.dh, B, n);
    GDL_CHECK_LAUNCH("film_dh_kernel");
    if (dWo && dbo) {
        hipLaunchKernelGGL(film_dwo_kernel, dim3(n), dim3(256), 0, st, hx, hf, hy, g_x_out, g_out, g_y_out, uni, dWo, dbo, B, n);
        GDL_CHECK_LAUNCH("film_dwo_kernel");
    }
    int rc;
    if (dx && dy) {
        hipLaunchKernelGGL(film_u_kernel<true>, dim3(4096), dim3(256), 0, st, w.dh, x, y, w.U, B, Bp);
        GDL_CHECK_LAUNCH("film_u_kernel");
        // out2[col][i] = sum_(k,j) U[(k,j)][col] A[(k,j)][i]
        rc = conv_wgrad(GDL_F32, w.U, Wfc, w.out2, w.tab_a, film_gemm(FD, 2 * Bp), FD, w.wg, w.wg_bytes, st);
        if (rc) return rc;
        hipLaunchKernelGGL(film_dxy_kernel, dim3(B, 2), dim3(256), 0, st, w.T, w.dh, w.out2, dx, dy, B, Bp);
        GDL_CHECK_LAUNCH("film_dxy_kernel");
    }
    if (dWfc && dbfc) {
        const int nblk = uni ? 3 : 1;
        hipLaunchKernelGGL(film_p_kernel, dim3(4096), dim3(256), 0, st, w.dh, x, y, w.P, B, Bp, nblk);
        GDL_CHECK_LAUNCH("film_p_kernel");
        hipLaunchKernelGGL(film_z_kernel, dim3(FD), dim3(128), 0, st, x, y, w.Z, B, Bp, nblk);
        GDL_CHECK_LAUNCH("film_z_kernel");
        rc = build_gather_table(GATHER_FWD, GDL_F32, film_gemm(nblk * Bp, FD), (GatherEntry*)w.tab_p, st);
        if (rc) return rc;
        // dA[(k,i)][j] = sum_c P[(k,i)][c] Z[j][c]
        rc = conv_fwd(GDL_F32, w.P, w.Z, dWfc, nullptr, w.tab_p, film_gemm(nblk * Bp, FD), st);
        if (rc) return rc;
        hipLaunchKernelGGL(film_dbfc_kernel, dim3(2), dim3(256), 0, st, w.dh, uni, dbfc, B);
        GDL_CHECK_LAUNCH("film_dbfc_kernel");
    }
    return GDL_OK;
}

// ---------------------------------------------------------------- FiLM, trained jointly (fusion_modules.py:91-124)
//   out = fc_out(fc(flatten(x (x) y))):  h_f[b][k] = x_b^T W_k y_b + bias_k  -- the fused form alone, nothing detached.
// T[(k,i)][b] = (W_k y_b)[i] is needed for the y columns only: Bj = B rounded up to 64 columns (the GEMMs' channel granule)
// against the DGL head's 2 * Bp -- half the f32 contraction over fc.weight at B = 64.  The workspace is the DGL head's
// (gdl_head_film_workspace_bytes), laid out by film_layout; the pieces are used with Bj columns:
//   V  [Bj][512] = y (padding rows zero)        T  [(k,i)][Bj]
//   dh [3][B][512], only the fused plane [1] carries values (film_p_kernel / film_dbfc_kernel index it that way)
//   U  [(k,i)][Bj] = dh[b][k] x_b[i]            out2 [Bj][512] = U^T A = dy
//   P  the weight-gradient GEMM's operand (Bp columns, as in the DGL head) -- and before it is written, the split
//      partials of the dy contraction (at most 27 MB of its >= 100 MB)
static inline int film_bj(int B) { return (B + 63) / 64 * 64; }

// dx[b][i] = sum_k dh_f[b][k] T[(k,i)][b]  (T is still in the workspace: no GEMM);  dy[b][i] = out2[b][i]
// grid = (512 i, ceil(B / 64)): a lane per sample (coalesced rows of T), four slices of k summed in a fixed order
__global__ __launch_bounds__(256) void film_joint_dxy_kernel(const float* __restrict__ T, const float* __restrict__ dhf,
                                                             const float* __restrict__ out2, float* __restrict__ dx,
                                                             float* __restrict__ dy, int B, int ld) {
    __shared__ float red[4][64];
    const int i = blockIdx.x;
    const int bl = threadIdx.x & 63, b = blockIdx.y * 64 + bl, part = threadIdx.x >> 6;
    float s = 0.f;
    if (b < B) {
        const float* Ti = T + (size_t)i * ld + b;
        for (int k = part; k < FD; k += 4) s = fmaf(dhf[(size_t)b * FD + k], Ti[(size_t)k * FD * ld], s);
    }
    red[part][bl] = s;
    __syncthreads();
    if (part == 0 && b < B) {
        dx[(size_t)b * FD + i] = ((red[0][bl] + red[1][bl]) + red[2][bl]) + red[3][bl];
        dy[(size_t)b * FD + i] = out2[(size_t)b * FD + i];
    }
}

// hidden: [B][512] = h_f (kept by the caller for the backward, together with ws: T is reused)
int head_film_joint_fwd(const float* x, const float* y, const float* Wfc, const float* bfc, const float* Wo, const float* bo,
                        float* hidden, float* out, int B, int n, void* ws, size_t ws_bytes, hipStream_t st) {
    GDL_REQUIRE(B >= 1 && B <= FILM_MAX_B, "head_film: B=%d (1..%d per call)", B, FILM_MAX_B);
    const FilmWs w = film_layout((unsigned char*)ws, B);
    if (!ws || ws_bytes < w.total) {
        set_error("head_film_joint_fwd: workspace %zu < %zu bytes", ws_bytes, w.total);
        return GDL_ERR_WORKSPACE;
    }
    const int Bj = film_bj(B);  // <= 2 * Bp: V, T, U and out2 of the DGL layout hold the Bj-column forms
    hipLaunchKernelGGL(film_v_kernel, dim3(Bj), dim3(256), 0, st, (const float*)nullptr, y, w.V, B, Bj, 1);
    GDL_CHECK_LAUNCH("film_v_kernel");
    int rc = build_gather_table(GATHER_FWD, GDL_F32, film_gemm(FD, Bj), (GatherEntry*)w.tab_a, st);
    if (rc) return rc;
    // T[(k,i)][b] = sum_j A[(k,i)][j] y_b[j]
    rc = conv_fwd(GDL_F32, Wfc, w.V, w.T, nullptr, w.tab_a, film_gemm(FD, Bj), st);
    if (rc) return rc;
    hipLaunchKernelGGL(film_h_kernel, dim3(FD, 1, (B + 63) / 64), dim3(256), 0, st, w.T, x, y, bfc, (float*)nullptr, hidden,
                       (float*)nullptr, B, Bj, 0, 1);
    GDL_CHECK_LAUNCH("film_h_kernel");
    hipLaunchKernelGGL(film_out_kernel<false>, dim3(B), dim3(256), 0, st, (const float*)nullptr, hidden, (const float*)nullptr, Wo,
                       bo, out, (float*)nullptr, (float*)nullptr, n);
    GDL_CHECK_LAUNCH("film_out_kernel");
    return GDL_OK;
}

// Needs the workspace of the matching joint forward untouched (T, the gather table).  dx/dy, dWfc/dbfc, dWo/dbo: optional pairs.
int head_film_joint_bwd(const float* x, const float* y, const float* Wfc, const float* Wo, const float* hidden, const float* g_out,
                        float* dx, float* dy, float* dWfc, float* dbfc, float* dWo, float* dbo, int B, int n, void* ws,
                        size_t ws_bytes, hipStream_t st) {
    GDL_REQUIRE(B >= 1 && B <= FILM_MAX_B, "head_film: B=%d (1..%d per call)", B, FILM_MAX_B);
    const FilmWs w = film_layout((unsigned char*)ws, B);
    if (!ws || ws_bytes < w.total) {
        set_error("head_film_joint_bwd: workspace %zu < %zu bytes", ws_bytes, w.total);
        return GDL_ERR_WORKSPACE;
    }
    const int Bp = film_bp(B), Bj = film_bj(B);
    const float* dhf = w.dh + (size_t)B * FD;
    // dh[1] = g_out Wo (the planes of the absent unimodal logit sets are written as zeros)
    hipLaunchKernelGGL(film_dh_kernel, dim3(B, 3), dim3(256), 0, st, (const float*)nullptr, g_out, (const float*)nullptr, Wo, w.dh, B, n);
    GDL_CHECK_LAUNCH("film_dh_kernel");
    if (dWo && dbo) {
        hipLaunchKernelGGL(film_dwo_kernel, dim3(n), dim3(256), 0, st, hidden, hidden, hidden, (const float*)nullptr, g_out,
                           (const float*)nullptr, 0, dWo, dbo, B, n);
        GDL_CHECK_LAUNCH("film_dwo_kernel");
    }
    int rc;
    if (dx && dy) {
        hipLaunchKernelGGL(film_u_kernel<false>, dim3(4096), dim3(256), 0, st, dhf, x, (const float*)nullptr, w.U, B, Bj);
        GDL_CHECK_LAUNCH("film_u_kernel");
        // out2[b][j] = sum_(k,i) U[(k,i)][b] A[(k,i)][j]; the split partials go to the (not yet written) P piece
        rc = conv_wgrad(GDL_F32, w.U, Wfc, w.out2, w.tab_a, film_gemm(FD, Bj), FD, w.P, (size_t)FROWS * 3 * Bp * 4, st);
        if (rc) return rc;
        hipLaunchKernelGGL(film_joint_dxy_kernel, dim3(FD, (B + 63) / 64), dim3(256), 0, st, w.T, dhf, w.out2, dx, dy, B, Bj);
        GDL_CHECK_LAUNCH("film_joint_dxy_kernel");
    }
    if (dWfc && dbfc) {  // the DGL head's phase-2 path: one block of Bp columns, P = dh_f (x) x, Z = y
        hipLaunchKernelGGL(film_p_kernel, dim3(4096), dim3(256), 0, st, w.dh, x, y, w.P, B, Bp, 1);
        GDL_CHECK_LAUNCH("film_p_kernel");
        hipLaunchKernelGGL(film_z_kernel, dim3(FD), dim3(128), 0, st, x, y, w.Z, B, Bp, 1);
        GDL_CHECK_LAUNCH("film_z_kernel");
        rc = build_gather_table(GATHER_FWD, GDL_F32, film_gemm(Bp, FD), (GatherEntry*)w.tab_p, st);
        if (rc) return rc;
        rc = conv_fwd(GDL_F32, w.P, w.Z, dWfc, nullptr, w.tab_p, film_gemm(Bp, FD), st);
        if (rc) return rc;
        hipLaunchKernelGGL(film_dbfc_kernel, dim3(2), dim3(256), 0, st, w.dh, 0, dbfc, B);
        GDL_CHECK_LAUNCH("film_dbfc_kernel");
    }
    return GDL_OK;
}


}  // namespace gdl
