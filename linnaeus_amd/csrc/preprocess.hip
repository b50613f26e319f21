// Image preprocessing on the device (inference/preprocessing.py:29-82 preprocess_single_image / preprocess_image_batch: per image
// TF.resize of a PIL image, TF.to_tensor, TF.normalize, then torch.stack and .cuda()): a batch of RGB uint8 images of different sizes
// -> fp32 [N, 3, H, W], in Pillow's own arithmetic (22-bit fixed point, int32 sums, a uint8 rounding between the passes), so that the
// result is the reference's bit for bit.  The work is bound by bytes -- the host-to-device copy of the sources costs more than both
// kernels -- so the kernels are plain: no float before the final normalize, byte loads along rows, tables and source segments in LDS.
//   resize_h_kernel      grid (image, group of PH_ROWS rows).  Only for images whose width changes, only the rows [y0, y0 + rows) the
//                        vertical pass will read.  The workgroup walks the output columns in tiles of at most PH_COLS; per tile and chunk
//                        of PP_CHUNK taps it stages the coefficient rows and, per source row, the byte segment the tile reads.
//   resize_v_kernel      grid (image, PV_ROWS output rows, PV_COLS columns).  Reads the intermediate, or the source itself where the width
//                        already fits; the same tiling turned by 90 degrees; then (u8 / 255 - mean) / std into the CHW plane, x fastest.
//                        An image whose height already fits skips the taps (a copy).
//   nearest_kernel       grid (image, output row, 256 columns): gather through the two index tables, normalize, store.
// A tile never covers more outputs than its staged segment can feed: with sc = ceil(in / out) >= scale, xmin(x) - xmin(x0) <=
// (x - x0) * sc + 1, so nx outputs and one chunk read at most (nx - 1) * sc + 1 + PP_CHUNK source positions from xmin(x0) + t0 on.
// Every global address comes from the descriptors, which lnx_preprocess has checked on the host; what the tables in the blob hold only
// selects positions inside staged LDS segments whose global range is clamped to the image.
#include <math.h>

#include <algorithm>

#include "common.hpp"
#include "../../include/lnx.h"

// ---------------------------------------------------------------------------------------------------------------------------------
// host: the tables of one axis, Pillow's precompute_coeffs / normalize_coeffs_8bpc (and the nearest walk of its affine transform)
// in the same order of double operations; nothing may be contracted into a multiply-add.
// ---------------------------------------------------------------------------------------------------------------------------------
#pragma clang fp contract(off)
namespace {

constexpr int PRECISION_BITS = 22;

double bilinear_filter(double x) {
    if (x < 0.0) x = -x;
    return x < 1.0 ? 1.0 - x : 0.0;
}
double bicubic_filter(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

struct Axis {
    double scale, fs, support;
    int taps;
    Axis(int in, int out, int filter) {
        scale = (double)in / out;
        fs = scale < 1.0 ? 1.0 : scale;
        support = (filter == LNX_RESIZE_BILINEAR ? 1.0 : 2.0) * fs;
        taps = (int)ceil(support) * 2 + 1;
    }
    void window(int in, int xx, int& xmin, int& n, double& center) const {
        center = (xx + 0.5) * scale;
        xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in) xmax = in;
        n = xmax - xmin;
    }
};

bool filter_ok(int f) { return f == LNX_RESIZE_NEAREST || f == LNX_RESIZE_BILINEAR || f == LNX_RESIZE_BICUBIC; }
bool side_ok(int s) { return s >= 1 && s <= LNX_PREPROCESS_MAX_SIDE; }
int64_t align16(int64_t v) { return (v + 15) & ~(int64_t)15; }

// the source rows [y0, y0 + rows) a vertical pass h -> H reads (bounds are monotonic: the first xmin, the last xmax)
void vertical_range(int h, int H, int filter, int& y0, int& rows) {
    if (h == H || filter == LNX_RESIZE_NEAREST) {
        y0 = 0;
        rows = h;
        return;
    }
    const Axis ax(h, H, filter);
    int xmin, n;
    double c;
    ax.window(h, 0, y0, n, c);
    ax.window(h, H - 1, xmin, n, c);
    rows = xmin + n - y0;
}

}  // namespace

extern "C" int lnx_resize_taps(int in_size, int out_size, int filter) {
    if (!filter_ok(filter) || !side_ok(in_size) || !side_ok(out_size)) {
        lnx_set_error("lnx_resize_taps: in=%d out=%d (1..%d) filter=%d (0 nearest, 1 bilinear, 2 bicubic)", in_size, out_size, LNX_PREPROCESS_MAX_SIDE, filter);
        return 0;
    }
    return filter == LNX_RESIZE_NEAREST ? 1 : Axis(in_size, out_size, filter).taps;
}

extern "C" int lnx_resize_coeffs(int in_size, int out_size, int filter, int32_t* k, int32_t* bounds) {
    LNX_CHECK(filter_ok(filter), "lnx_resize_coeffs: filter=%d (0 nearest, 1 bilinear, 2 bicubic)", filter);
    LNX_CHECK(side_ok(in_size) && side_ok(out_size), "lnx_resize_coeffs: in=%d out=%d (1..%d)", in_size, out_size, LNX_PREPROCESS_MAX_SIDE);
    LNX_CHECK(bounds, "lnx_resize_coeffs: NULL bounds");
    if (filter == LNX_RESIZE_NEAREST) {
        const double a = (double)in_size / out_size;
        double xo = a * 0.5;
        for (int xx = 0; xx < out_size; ++xx) {
            const int x = (int)xo;
            bounds[xx] = x < in_size - 1 ? x : in_size - 1;
            xo += a;
        }
        return 0;
    }
    LNX_CHECK(k, "lnx_resize_coeffs: NULL k");
    const Axis ax(in_size, out_size, filter);
    const double ss = 1.0 / ax.fs;
    double* w = new double[ax.taps];
    for (int xx = 0; xx < out_size; ++xx) {
        int xmin, n;
        double center;
        ax.window(in_size, xx, xmin, n, center);
        double ww = 0.0;
        for (int x = 0; x < n; ++x) {
            const double t = (x + xmin - center + 0.5) * ss;
            w[x] = filter == LNX_RESIZE_BILINEAR ? bilinear_filter(t) : bicubic_filter(t);
            ww += w[x];
        }
        int32_t* kk = k + (int64_t)xx * ax.taps;
        for (int x = 0; x < n; ++x) {
            if (ww != 0.0) w[x] /= ww;
            kk[x] = w[x] < 0 ? (int)(-0.5 + w[x] * (1 << PRECISION_BITS)) : (int)(0.5 + w[x] * (1 << PRECISION_BITS));
        }
        for (int x = n; x < ax.taps; ++x) kk[x] = 0;
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = n;
    }
    delete[] w;
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// device
// ---------------------------------------------------------------------------------------------------------------------------------
namespace {

constexpr int PP_THREADS = 256;
constexpr int PP_CHUNK = 64;          // taps per staged chunk
constexpr int PP_KLD = PP_CHUNK + 1;  // row stride of the staged coefficients (odd: neighbouring outputs fall on different banks)
constexpr int PH_ROWS = 4, PH_COLS = 64, PH_SEG = 1024;  // horizontal: rows x output columns of a tile, source pixels staged per row
constexpr int PV_ROWS = 8, PV_COLS = 64, PV_SEG = 96;    // vertical: output rows x columns of a tile, source rows staged
constexpr int PH_OUT = PH_ROWS * PH_COLS * 3 / PP_THREADS;  // outputs per thread and tile
constexpr int PV_OUT = PV_ROWS * PV_COLS * 3 / PP_THREADS;
static_assert(PH_ROWS * PH_COLS * 3 % PP_THREADS == 0 && PV_ROWS * PV_COLS * 3 % PP_THREADS == 0, "whole outputs per thread");
static_assert(PH_SEG > PP_CHUNK + 1 && PV_SEG > PP_CHUNK + 1, "a tile of one output always fits");

struct PreParams {
    const uint8_t* blob;
    uint8_t* scratch;
    int64_t images_off;
    int H, W;
    float mean[3], std[3];
    float* out;
};

__device__ __forceinline__ const lnx_preprocess_image& image_of(const PreParams& p, int i) {
    return reinterpret_cast<const lnx_preprocess_image*>(p.blob + p.images_off)[i];
}
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ float normalized(int u8, float mean, float std) { return ((float)u8 / 255.0f - mean) / std; }

__global__ __launch_bounds__(PP_THREADS) void resize_h_kernel(const PreParams p) {
    __shared__ int32_t sk[PH_COLS * PP_KLD];
    __shared__ int32_t sb[PH_COLS * 2];
    __shared__ uint8_t ss[PH_ROWS][PH_SEG * 3];
    const lnx_preprocess_image d = image_of(p, blockIdx.x);
    const int W = p.W, tid = threadIdx.x;
    const int ra = blockIdx.y * PH_ROWS;
    if (d.w == W || ra >= d.rows) return;  // (uniform over the workgroup)
    const int nr = min(PH_ROWS, d.rows - ra);
    const uint8_t* src = p.blob + d.src + (int64_t)(d.y0 + ra) * d.w * 3;
    uint8_t* dst = p.scratch + d.scratch + (int64_t)ra * W * 3;
    const int32_t* K = reinterpret_cast<const int32_t*>(p.blob + d.hk);
    const int32_t* B = reinterpret_cast<const int32_t*>(p.blob + d.hb);
    const int sc = (d.w + W - 1) / W;
    const int xt = min(PH_COLS, 1 + (PH_SEG - PP_CHUNK - 1) / sc);
    for (int x0 = 0; x0 < W; x0 += xt) {
        const int nx = min(xt, W - x0);
        __syncthreads();  // the tile before is done with sb, sk and ss
        for (int i = tid; i < nx * 2; i += PP_THREADS) sb[i] = B[x0 * 2 + i];
        __syncthreads();
        const int first = sb[0];
        int acc[PH_OUT], r_[PH_OUT], x_[PH_OUT], c_[PH_OUT], lo_[PH_OUT], n_[PH_OUT];
#pragma unroll
        for (int j = 0; j < PH_OUT; ++j) {
            const int o = tid + j * PP_THREADS;
            r_[j] = o / (nx * 3);
            const int rem = o - r_[j] * nx * 3;
            x_[j] = rem / 3;
            c_[j] = rem - x_[j] * 3;
            const bool live = r_[j] < nr;
            lo_[j] = live ? sb[2 * x_[j]] : 0;
            n_[j] = live ? sb[2 * x_[j] + 1] : 0;
            acc[j] = 1 << 21;
        }
        for (int t0 = 0; t0 < d.htaps; t0 += PP_CHUNK) {
            const int tc = min(PP_CHUNK, d.htaps - t0);
            const int seg0 = clampi(first + t0, 0, d.w);
            const int segn = max(0, min((nx - 1) * sc + 1 + PP_CHUNK, d.w - seg0));
            if (t0 > 0) __syncthreads();  // the chunk before is done with sk and ss
            for (int i = tid; i < nx * tc; i += PP_THREADS) {
                const int x = i / tc, t = i - x * tc;
                sk[x * PP_KLD + t] = K[(int64_t)(x0 + x) * d.htaps + t0 + t];
            }
            for (int r = 0; r < nr; ++r) {
                const uint8_t* row = src + (int64_t)r * d.w * 3 + (int64_t)seg0 * 3;
                for (int i = tid; i < segn * 3; i += PP_THREADS) ss[r][i] = row[i];
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < PH_OUT; ++j) {
                const int lim = min(tc, n_[j] - t0);
                const uint8_t* s = &ss[r_[j] < nr ? r_[j] : 0][(lo_[j] + t0 - seg0) * 3 + c_[j]];
                const int32_t* k = &sk[x_[j] * PP_KLD];
                for (int t = 0; t < lim; ++t) acc[j] += (int)s[3 * t] * k[t];
            }
        }
#pragma unroll
        for (int j = 0; j < PH_OUT; ++j)
            if (r_[j] < nr) dst[(int64_t)r_[j] * W * 3 + (x0 + x_[j]) * 3 + c_[j]] = (uint8_t)clampi(acc[j] >> PRECISION_BITS, 0, 255);
    }
}

__global__ __launch_bounds__(PP_THREADS) void resize_v_kernel(const PreParams p) {
    __shared__ int32_t sk[PV_ROWS * PP_KLD];
    __shared__ int32_t sb[PV_ROWS * 2];
    __shared__ uint8_t ss[PV_SEG][PV_COLS * 3];
    const int img = blockIdx.x;
    const lnx_preprocess_image d = image_of(p, img);
    const int H = p.H, W = p.W, tid = threadIdx.x;
    const int xa = blockIdx.z * PV_COLS, nx = min(PV_COLS, W - xa);
    const int yb = blockIdx.y * PV_ROWS, ye = min(H, yb + PV_ROWS);
    // the plane the pass reads: [prows, W, 3] starting at source row py0
    const bool from_src = d.w == W;
    const uint8_t* plane = from_src ? p.blob + d.src : p.scratch + d.scratch;
    const int py0 = from_src ? 0 : d.y0, prows = from_src ? d.h : d.rows;
    const bool copy = d.h == H;
    const int32_t* K = reinterpret_cast<const int32_t*>(p.blob + d.vk);
    const int32_t* B = reinterpret_cast<const int32_t*>(p.blob + d.vb);
    const int sc = (d.h + H - 1) / H;
    const int yt = min(PV_ROWS, 1 + (PV_SEG - PP_CHUNK - 1) / sc);
    const int vtaps = copy ? 0 : d.vtaps;
    for (int ya = yb; ya < ye; ya += yt) {
        const int ny = min(yt, ye - ya);
        int first = 0;
        if (!copy) {
            __syncthreads();  // the rows before are done with sb, sk and ss
            for (int i = tid; i < ny * 2; i += PP_THREADS) sb[i] = B[ya * 2 + i];
            __syncthreads();
            first = sb[0];
        }
        int acc[PV_OUT], y_[PV_OUT], lo_[PV_OUT], n_[PV_OUT];
        const int x = tid & (PV_COLS - 1);
        bool live[PV_OUT];
#pragma unroll
        for (int j = 0; j < PV_OUT; ++j) {  // o = tid + j * 256 -> (y, c, x), x fastest: thread's x is fixed, (y, c) = (o / 192, o % 192 / 64)
            const int o = tid + j * PP_THREADS;
            y_[j] = o / (PV_COLS * 3);
            live[j] = y_[j] < ny && x < nx;
            lo_[j] = live[j] && !copy ? sb[2 * y_[j]] : 0;
            n_[j] = live[j] && !copy ? sb[2 * y_[j] + 1] : 0;
            acc[j] = 1 << 21;
        }
        for (int t0 = 0; t0 < vtaps; t0 += PP_CHUNK) {
            const int tc = min(PP_CHUNK, vtaps - t0);
            const int r0 = clampi(first + t0 - py0, 0, prows);
            const int rn = max(0, min((ny - 1) * sc + 1 + PP_CHUNK, prows - r0));
            if (t0 > 0) __syncthreads();  // the chunk before is done with sk and ss
            for (int i = tid; i < ny * tc; i += PP_THREADS) {
                const int y = i / tc, t = i - y * tc;
                sk[y * PP_KLD + t] = K[(int64_t)(ya + y) * vtaps + t0 + t];
            }
            for (int i = tid; i < rn * nx * 3; i += PP_THREADS) {
                const int r = i / (nx * 3), b = i - r * nx * 3;
                ss[r][b] = plane[((int64_t)(r0 + r) * W + xa) * 3 + b];
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < PV_OUT; ++j) {
                const int c = (tid + j * PP_THREADS) % (PV_COLS * 3) / PV_COLS;
                const int lim = min(tc, n_[j] - t0);
                const uint8_t* s = &ss[0][0] + (lo_[j] + t0 - py0 - r0) * (PV_COLS * 3) + x * 3 + c;
                const int32_t* k = &sk[(live[j] ? y_[j] : 0) * PP_KLD];
                for (int t = 0; t < lim; ++t) acc[j] += (int)s[t * (PV_COLS * 3)] * k[t];
            }
        }
#pragma unroll
        for (int j = 0; j < PV_OUT; ++j) {
            if (!live[j]) continue;
            const int c = (tid + j * PP_THREADS) % (PV_COLS * 3) / PV_COLS;
            const int y = ya + y_[j];
            const int u8 = copy ? (int)plane[((int64_t)y * W + xa + x) * 3 + c] : clampi(acc[j] >> PRECISION_BITS, 0, 255);
            p.out[(((int64_t)img * 3 + c) * H + y) * W + xa + x] = normalized(u8, p.mean[c], p.std[c]);
        }
    }
}

__global__ __launch_bounds__(PP_THREADS) void nearest_kernel(const PreParams p) {
    const int img = blockIdx.x, y = blockIdx.y, x = blockIdx.z * PP_THREADS + threadIdx.x;
    if (x >= p.W) return;
    const lnx_preprocess_image& d = image_of(p, img);
    const int sy = clampi(reinterpret_cast<const int32_t*>(p.blob + d.vb)[y], 0, d.h - 1);
    const int sx = clampi(reinterpret_cast<const int32_t*>(p.blob + d.hb)[x], 0, d.w - 1);
    const uint8_t* s = p.blob + d.src + ((int64_t)sy * d.w + sx) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) p.out[(((int64_t)img * 3 + c) * p.H + y) * p.W + x] = normalized(s[c], p.mean[c], p.std[c]);
}

// what lnx_preprocess_scratch_bytes writes into a descriptor, from its h and w; the scratch offset is the caller's running sum
struct Derived {
    int htaps, vtaps, y0, rows;
    int64_t scratch_bytes;
};
Derived derive(int h, int w, int H, int W, int filter) {
    Derived r;
    const bool interp = filter != LNX_RESIZE_NEAREST;
    r.htaps = interp && w != W ? lnx_resize_taps(w, W, filter) : 0;
    r.vtaps = interp && h != H ? lnx_resize_taps(h, H, filter) : 0;
    vertical_range(h, H, filter, r.y0, r.rows);
    r.scratch_bytes = interp && w != W ? align16((int64_t)r.rows * W * 3) : 0;
    return r;
}

}  // namespace

extern "C" int64_t lnx_preprocess_scratch_bytes(lnx_preprocess_image* images, int n, int H, int W, int filter) {
#define PRE_REFUSE(cond, ...)            \
    do {                                 \
        if (!(cond)) {                   \
            lnx_set_error(__VA_ARGS__);  \
            return -1;                   \
        }                                \
    } while (0)
    PRE_REFUSE(images, "lnx_preprocess_scratch_bytes: NULL images");
    PRE_REFUSE(n > 0, "lnx_preprocess_scratch_bytes: n=%d", n);
    PRE_REFUSE(side_ok(H) && side_ok(W), "lnx_preprocess_scratch_bytes: output side H=%d W=%d (1..%d)", H, W, LNX_PREPROCESS_MAX_SIDE);
    PRE_REFUSE(filter_ok(filter), "lnx_preprocess_scratch_bytes: unknown filter=%d (0 nearest, 1 bilinear, 2 bicubic)", filter);
    int64_t total = 0;
    for (int i = 0; i < n; ++i) {
        lnx_preprocess_image& d = images[i];
        PRE_REFUSE(side_ok(d.h) && side_ok(d.w), "lnx_preprocess_scratch_bytes: image %d has source side h=%d w=%d (1..%d)", i, d.h, d.w, LNX_PREPROCESS_MAX_SIDE);
        const Derived r = derive(d.h, d.w, H, W, filter);
        d.htaps = r.htaps;
        d.vtaps = r.vtaps;
        d.y0 = r.y0;
        d.rows = r.rows;
        d.scratch = total;
        total += r.scratch_bytes;
    }
    return total;
#undef PRE_REFUSE
}

extern "C" int lnx_preprocess(const lnx_preprocess_args* a, void* stream) {
    LNX_CHECK(a, "lnx_preprocess: NULL arguments");
    LNX_CHECK(a->n > 0, "lnx_preprocess: n=%d", a->n);
    LNX_CHECK(side_ok(a->H) && side_ok(a->W), "lnx_preprocess: output side H=%d W=%d (1..%d)", a->H, a->W, LNX_PREPROCESS_MAX_SIDE);
    LNX_CHECK(filter_ok(a->filter), "lnx_preprocess: unknown filter=%d (0 nearest, 1 bilinear, 2 bicubic)", a->filter);
    LNX_CHECK(a->images && a->blob && a->out, "lnx_preprocess: NULL pointer (images / blob / out)");
    LNX_CHECK((reinterpret_cast<uintptr_t>(a->blob) & 15) == 0, "lnx_preprocess: blob is not 16-byte aligned");
    for (int c = 0; c < 3; ++c) LNX_CHECK(a->std[c] != 0.0f, "lnx_preprocess: std[%d] == 0", c);
    const int H = a->H, W = a->W;
    const int64_t nb = a->blob_bytes;
    LNX_CHECK(a->images_off >= 0 && (a->images_off & 7) == 0 && a->images_off <= nb && (int64_t)a->n * (int64_t)sizeof(lnx_preprocess_image) <= nb - a->images_off,
              "lnx_preprocess: descriptor table at %lld (a multiple of 8) with %d entries does not fit the blob of %lld bytes", (long long)a->images_off, a->n, (long long)nb);
    LNX_CHECK(a->scratch_bytes >= 0, "lnx_preprocess: scratch_bytes=%lld", (long long)a->scratch_bytes);
    auto inside = [nb](int64_t off, int64_t bytes, int64_t align) { return off >= 0 && (off & (align - 1)) == 0 && off <= nb && bytes <= nb - off; };
    bool any_h = false;
    int max_groups = 0;
    for (int i = 0; i < a->n; ++i) {
        const lnx_preprocess_image& d = a->images[i];
        LNX_CHECK(side_ok(d.h) && side_ok(d.w), "lnx_preprocess: image %d has source side h=%d w=%d (1..%d)", i, d.h, d.w, LNX_PREPROCESS_MAX_SIDE);
        const Derived r = derive(d.h, d.w, H, W, a->filter);
        LNX_CHECK(d.htaps == r.htaps && d.vtaps == r.vtaps && d.y0 == r.y0 && d.rows == r.rows,
                  "lnx_preprocess: image %d (%dx%d) carries htaps=%d vtaps=%d y0=%d rows=%d, expected %d %d %d %d (lnx_preprocess_scratch_bytes sets them)", i, d.h, d.w,
                  d.htaps, d.vtaps, d.y0, d.rows, r.htaps, r.vtaps, r.y0, r.rows);
        LNX_CHECK(inside(d.src, (int64_t)d.h * d.w * 3, 1), "lnx_preprocess: image %d source at %lld leaves the blob of %lld bytes", i, (long long)d.src, (long long)nb);
        if (a->filter == LNX_RESIZE_NEAREST) {
            LNX_CHECK(inside(d.hb, (int64_t)W * 4, 4) && inside(d.vb, (int64_t)H * 4, 4), "lnx_preprocess: image %d index tables leave the blob or are not 4-byte aligned", i);
            continue;
        }
        if (r.htaps)
            LNX_CHECK(inside(d.hk, (int64_t)W * r.htaps * 4, 4) && inside(d.hb, (int64_t)W * 8, 4), "lnx_preprocess: image %d horizontal tables leave the blob or are not 4-byte aligned", i);
        if (r.vtaps)
            LNX_CHECK(inside(d.vk, (int64_t)H * r.vtaps * 4, 4) && inside(d.vb, (int64_t)H * 8, 4), "lnx_preprocess: image %d vertical tables leave the blob or are not 4-byte aligned", i);
        if (r.scratch_bytes) {
            LNX_CHECK(a->scratch, "lnx_preprocess: NULL scratch, image %d needs %lld bytes", i, (long long)r.scratch_bytes);
            LNX_CHECK(d.scratch >= 0 && d.scratch <= a->scratch_bytes && r.scratch_bytes <= a->scratch_bytes - d.scratch,
                      "lnx_preprocess: scratch too small: image %d needs %lld bytes at %lld, scratch_bytes=%lld", i, (long long)r.scratch_bytes, (long long)d.scratch,
                      (long long)a->scratch_bytes);
            any_h = true;
            max_groups = std::max(max_groups, cdiv(r.rows, PH_ROWS));
        }
    }
    PreParams p;
    p.blob = static_cast<const uint8_t*>(a->blob);
    p.scratch = static_cast<uint8_t*>(a->scratch);
    p.images_off = a->images_off;
    p.H = H;
    p.W = W;
    for (int c = 0; c < 3; ++c) {
        p.mean[c] = a->mean[c];
        p.std[c] = a->std[c];
    }
    p.out = a->out;
    hipStream_t st = (hipStream_t)stream;
    if (a->filter == LNX_RESIZE_NEAREST) {
        hipLaunchKernelGGL(nearest_kernel, dim3(a->n, H, cdiv(W, PP_THREADS)), dim3(PP_THREADS), 0, st, p);
        LNX_LAUNCH_CHECK();
        return 0;
    }
    if (any_h) {
        hipLaunchKernelGGL(resize_h_kernel, dim3(a->n, max_groups), dim3(PP_THREADS), 0, st, p);
        LNX_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(resize_v_kernel, dim3(a->n, cdiv(H, PV_ROWS), cdiv(W, PV_COLS)), dim3(PP_THREADS), 0, st, p);
    LNX_LAUNCH_CHECK();
    return 0;
}
