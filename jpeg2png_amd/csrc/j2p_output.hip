// jpeg2png_amd — the output stage: solved planes to samples on the host (PNG), to a strided tensor in device memory, whole
// or cropped and resized (area, or triangle / cubic taps; several such outputs in one call), to quantised JPEG
// coefficients, and to the entropy-coded JPEG file itself (include/jpeg2png_amd.h: the j2p_planes_* functions, j2p_entropy_encode).
// And, because it shares that file's scan kernels, the way back: a JPEG file's entropy-coded data to coefficients
// (j2p_entropy_decode, j2p_decode_file; j2p_decode_kernels.hip.h).
//
// A translation unit of its own, with its own device code (j2p_output_kernels.hip.h): it changes more often than the solver
// and must not recompile the solver's kernels.  It sees of a solver what j2p_solver_view and j2p_solver_row give
// (j2p_internal.h), never the solver's struct, its halo or its arena; j2p_solver_scratch lends it memory that lives with the
// solver.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <chrono>

#include "jpeg2png_amd.h"
#include "j2p_internal.h"
#include "j2p_hip_host.h"
#include "j2p_output_kernels.hip.h"
#include "j2p_decode_kernels.hip.h"

using namespace j2p;

extern "C" {

// What the conversions of solved planes start from: rows [y0, y1) x w columns of the image from nplane (3 or 1) (solver,
// channel) pairs on one device that all hold those canvas rows.  Checks arguments and state, gives per plane the first of
// those rows in the current iterate and its stride in floats and the view of planes[0].solver, and waits for the streams of
// the other solvers: the caller launches on planes[0].solver's.  `whole`: called as a whole-canvas form, which band solvers
// refuse.  what: "to_rgb", "to_grey" or "to_tensor", for the messages.
static int resolve_rows(const char *what, const j2p_plane_ref *planes, unsigned nplane, bool whole, unsigned w, unsigned y0, unsigned y1,
                        const float *ptr[3], unsigned stride[3], j2p_solver_view &first)
{
        if(w == 0 || y0 >= y1) { return j2p_fail(J2P_EINVAL, whole ? "empty image" : "empty row range"); }
        for(unsigned i = 0; whole && i < nplane; i++) {
                if(planes[i].solver && !j2p_solver_view_of(planes[i].solver).whole) {
                        return j2p_fail(J2P_ESTATE, "%s needs whole-canvas solvers (bands: j2p_planes_rows_%s)", what, what);
                }
        }
        for(unsigned i = 0; i < 3; i++) { ptr[i] = nullptr; stride[i] = 0; }
        for(unsigned i = 0; i < nplane; i++) {
                const j2p_solver_view s = planes[i].solver ? j2p_solver_view_of(planes[i].solver) : j2p_solver_view{};
                if(!planes[i].solver || planes[i].channel >= s.nch) { return j2p_fail(J2P_EINVAL, "plane %u: bad solver/channel", i); }
                if(i == 0) { first = s; }
                if(s.device != first.device) { return j2p_fail(J2P_EINVAL, "planes live on different devices"); }
                if(s.W < w || y0 < s.row0 || y1 > s.row0 + s.rows) {
                        return j2p_fail(J2P_EINVAL, "plane %u: rows [%u,%u) x %u columns are not inside the solver's [%u,%u) x %u", i, y0, y1, w,
                                    s.row0, s.row0 + s.rows, s.W);
                }
                if(s.mid_iteration) { return j2p_fail(J2P_ESTATE, "%s between the two phases of an iteration", what); }
                if(const int rc = j2p_solver_row(planes[i].solver, planes[i].channel, y0, &ptr[i]); rc != J2P_OK) { return rc; }
                stride[i] = s.W;
        }
        DeviceGuard guard(first.device);
        for(unsigned i = 1; i < nplane; i++) {
                if(planes[i].solver != planes[0].solver) { HIP_TRY(hipStreamSynchronize(j2p_solver_view_of(planes[i].solver).stream)); }
        }
        return J2P_OK;
}

// rows [y0, y1) of the image as samples on the host, through k_to_samples: three planes -> RGB, one -> greyscale
static int convert_rows(const j2p_plane_ref *planes, unsigned nplane, bool whole, unsigned w, unsigned y0, unsigned y1, unsigned bits,
                        uint8_t *out_host)
{
        const char *what = nplane == 3 ? "to_rgb" : "to_grey";
        if(!planes || !out_host) { return j2p_fail(J2P_EINVAL, "NULL argument"); }
        if(bits != 8 && bits != 16) { return j2p_fail(J2P_EINVAL, "bits must be 8 or 16 (png.c:22)"); }
        const float *ptr[3];
        unsigned stride[3];
        j2p_solver_view s0;
        if(const int rc = resolve_rows(what, planes, nplane, whole, w, y0, y1, ptr, stride, s0); rc != J2P_OK) { return rc; }
        const unsigned h = y1 - y0;
        DeviceGuard guard(s0.device);
        const size_t bytes = (size_t)w * h * (size_t)nplane * (bits / 8);
        void *dout = nullptr;
        size_t dout_bytes = 0;
        HIP_TRY(j2p_pool_take(s0.device, bytes, &dout, &dout_bytes));       // pooled like the solvers' arenas: no hipFree per image
        hipLaunchKernelGGL(nplane == 3 ? k_to_samples<3> : k_to_samples<1>, dim3(2048), dim3(256), 0, s0.stream, ptr[0], stride[0],
                           ptr[1], stride[1], ptr[2], stride[2], w, h, bits, static_cast<uint8_t *>(dout));
        hipError_t e = hipMemcpyAsync(out_host, dout, bytes, hipMemcpyDeviceToHost, s0.stream);
        if(e == hipSuccess) { e = hipStreamSynchronize(s0.stream); }
        j2p_pool_give(s0.device, dout, dout_bytes);
        if(e != hipSuccess) { return j2p_fail(J2P_EDEVICE, "planes_%s: %s", what, hipGetErrorString(e)); }
        return J2P_OK;
}

int j2p_planes_to_rgb(const j2p_plane_ref planes[3], unsigned w, unsigned h, unsigned bits, uint8_t *out_host)
{
        return convert_rows(planes, 3, true, w, 0, h, bits, out_host);
}

int j2p_planes_rows_to_rgb(const j2p_plane_ref planes[3], unsigned w, unsigned row_begin, unsigned row_end, unsigned bits,
                           uint8_t *out_host)
{
        return convert_rows(planes, 3, false, w, row_begin, row_end, bits, out_host);
}

int j2p_planes_to_grey(const j2p_plane_ref *plane, unsigned w, unsigned h, unsigned bits, uint8_t *out_host)
{
        return convert_rows(plane, 1, true, w, 0, h, bits, out_host);
}

int j2p_planes_rows_to_grey(const j2p_plane_ref *plane, unsigned w, unsigned row_begin, unsigned row_end, unsigned bits,
                            uint8_t *out_host)
{
        return convert_rows(plane, 1, false, w, row_begin, row_end, bits, out_host);
}

// ---- tensor output: k_to_tensor ----
static_assert(J2P_DTYPE_U8 == kDtypeU8 && J2P_DTYPE_F16 == kDtypeF16 && J2P_DTYPE_BF16 == kDtypeBF16 && J2P_DTYPE_F32 == kDtypeF32,
              "the kernels' dtype codes are the header's");

// Which destination path the full groups of 4 pixels of a w-column image take — the only place that knows the rule.  A
// vector path stores 4 elements at once, 16 / 8 / 4 bytes for f32 / 16-bit / u8, and needs every such store aligned to its
// width: the first row's address, and (in elements) the row stride and — planar, three planes — the channel stride multiples
// of 4; a lane's first column is a multiple of 4 already.  Everything else, and every image narrower than one group, is
// generic: correct for any strides, one element per store.  Decided per image, not per row: rows [a, b) of an image start
// at a multiple of stride_y from its first row, so the bands of one image agree.
static int tensor_path(unsigned w, unsigned nplane, int dtype, long long stride_c, long long stride_y, long long stride_x, uintptr_t address)
{
        const unsigned store_bytes = 4 * j2p_tensor_element_bytes(dtype);
        if(w < 4 || address % store_bytes != 0 || stride_y % 4 != 0) { return kTensorGeneric; }
        if(stride_x == 1 && (nplane == 1 || stride_c % 4 == 0)) { return kTensorPlanar; }
        if(nplane == 3 && stride_c == 1 && stride_x == 3) { return kTensorInterleaved; }
        return kTensorGeneric;
}

int j2p_debug_tensor_path(unsigned w, unsigned nplane, int dtype, ptrdiff_t stride_c, ptrdiff_t stride_y, ptrdiff_t stride_x,
                          uintptr_t data_address, int *path)
{
        if(!path || (nplane != 1 && nplane != 3) || dtype < J2P_DTYPE_U8 || dtype > J2P_DTYPE_F32 || w == 0 || stride_c < 1 || stride_y < 1 ||
           stride_x < 1) {
                return j2p_fail(J2P_EINVAL, "bad argument");
        }
        *path = tensor_path(w, nplane, dtype, stride_c, stride_y, stride_x, data_address);
        return J2P_OK;
}

using TensorKernel = void (*)(const float *, unsigned, const float *, unsigned, const float *, unsigned, unsigned, unsigned, TensorOut);

// [three planes / one][dtype][path]; one plane has no interleaved layout (tensor_path never chooses it there)
#define J2P_TENSOR_ROW(NPLANE, DTYPE, THIRD) {k_to_tensor<NPLANE, DTYPE, kTensorGeneric>, k_to_tensor<NPLANE, DTYPE, kTensorPlanar>, THIRD}
#define J2P_TENSOR_ROWS(NPLANE, THIRD)                                                                                                     \
        {J2P_TENSOR_ROW(NPLANE, kDtypeU8, THIRD(kDtypeU8)), J2P_TENSOR_ROW(NPLANE, kDtypeF16, THIRD(kDtypeF16)),                               \
         J2P_TENSOR_ROW(NPLANE, kDtypeBF16, THIRD(kDtypeBF16)), J2P_TENSOR_ROW(NPLANE, kDtypeF32, THIRD(kDtypeF32))}
#define J2P_TENSOR_INTERLEAVED(DTYPE) k_to_tensor<3, DTYPE, kTensorInterleaved>
#define J2P_TENSOR_NONE(DTYPE) nullptr
static const TensorKernel kTensorKernels[2][4][3] = {J2P_TENSOR_ROWS(3, J2P_TENSOR_INTERLEAVED), J2P_TENSOR_ROWS(1, J2P_TENSOR_NONE)};
#undef J2P_TENSOR_NONE
#undef J2P_TENSOR_INTERLEAVED
#undef J2P_TENSOR_ROWS
#undef J2P_TENSOR_ROW

// What both tensor outputs check before they launch, in this order: the arguments, the solvers' state and rows (resolve_rows),
// the 16-byte alignment of the canvas rows, and the destination's dtype, strides, address, scale / bias and device.  Gives the
// planes' first rows and strides, the kernels' view of the destination and the view of planes[0].solver.
static int tensor_resolve(const j2p_plane_ref *planes, unsigned nplane, bool whole, unsigned w, unsigned y0, unsigned y1, const j2p_tensor *out,
                          const float *ptr[3], unsigned stride[3], TensorOut &o, j2p_solver_view &s0)
{
        if(!planes || !out) { return j2p_fail(J2P_EINVAL, "NULL argument"); }
        if(nplane != 1 && nplane != 3) { return j2p_fail(J2P_EINVAL, "to_tensor: three planes (RGB) or one (greyscale), not %u", nplane); }
        if(const int rc = resolve_rows("to_tensor", planes, nplane, whole, w, y0, y1, ptr, stride, s0); rc != J2P_OK) { return rc; }
        for(unsigned i = 0; i < nplane; i++) {
                // what k_to_tensor's 16-byte loads rest on (see there): true of every solver j2p_solver_create makes
                if(stride[i] % 4 != 0 || reinterpret_cast<uintptr_t>(ptr[i]) % 16 != 0) { return j2p_fail(J2P_ESTATE, "plane %u: canvas rows are not 16-byte aligned", i); }
        }
        if(out->dtype != J2P_DTYPE_U8 && out->dtype != J2P_DTYPE_F16 && out->dtype != J2P_DTYPE_BF16 && out->dtype != J2P_DTYPE_F32) {
                return j2p_fail(J2P_EINVAL, "to_tensor: unknown dtype %d", out->dtype);
        }
        if(out->stride_c < 1 || out->stride_y < 1 || out->stride_x < 1) {
                return j2p_fail(J2P_EINVAL, "to_tensor: strides (%td, %td, %td) must all be at least 1 element", out->stride_c, out->stride_y, out->stride_x);
        }
        if(!out->data) { return j2p_fail(J2P_EINVAL, "to_tensor: data is NULL"); }
        if(reinterpret_cast<uintptr_t>(out->data) % j2p_tensor_element_bytes(out->dtype) != 0) {
                return j2p_fail(J2P_EINVAL, "to_tensor: data is not aligned to the %u-byte element", j2p_tensor_element_bytes(out->dtype));
        }
        o.data = out->data;
        o.stride_c = out->stride_c;
        o.stride_y = out->stride_y;
        o.stride_x = out->stride_x;
        for(unsigned k = 0; k < 3; k++) {
                // (one plane: only entry 0 is used, the others are not looked at)
                const float sc = k < nplane ? out->scale[k] : 1.f, bi = k < nplane ? out->bias[k] : 0.f;
                if(!__builtin_isfinite(sc) || !__builtin_isfinite(bi)) { return j2p_fail(J2P_EINVAL, "to_tensor: scale / bias of channel %u is not finite", k); }
                if(out->dtype == J2P_DTYPE_U8 && (sc != 1.f || bi != 0.f)) {
                        return j2p_fail(J2P_EINVAL, "to_tensor: u8 elements are the 8-bit samples: scale must be 1 and bias 0 (channel %u)", k);
                }
                o.scale[k] = sc;
                o.bias[k] = bi;
        }
        DeviceGuard guard(s0.device);
        {
                int device = -1;
                if(j2p_device_of_pointer(out->data, &device) != J2P_OK || device != s0.device) {
                        return j2p_fail(J2P_EINVAL, "to_tensor: data is not device memory of the solvers' device %d (managed and host memory are refused)", s0.device);
                }
        }
        return J2P_OK;
}

// rows [y0, y1) of the image from nplane (3 or 1) (solver, channel) pairs on one device into a strided tensor in that device's
// memory, through k_to_tensor; out->data is the element of row y0.  Asynchronous: the kernel is queued on planes[0].solver's
// stream and nothing waits for it.
static int tensor_rows(const j2p_plane_ref *planes, unsigned nplane, bool whole, unsigned w, unsigned y0, unsigned y1, const j2p_tensor *out)
{
        const float *ptr[3];
        unsigned stride[3];
        TensorOut o;
        j2p_solver_view s0;
        if(const int rc = tensor_resolve(planes, nplane, whole, w, y0, y1, out, ptr, stride, o, s0); rc != J2P_OK) { return rc; }
        DeviceGuard guard(s0.device);
        const unsigned h = y1 - y0;
        const int path = tensor_path(w, nplane, out->dtype, out->stride_c, out->stride_y, out->stride_x, reinterpret_cast<uintptr_t>(out->data));
        const TensorKernel kernel = kTensorKernels[nplane == 3 ? 0 : 1][out->dtype][path];
        // a workgroup: 4 rows of 256 columns; grid-stride over rows from a grid of about 2048 workgroups, as k_to_samples'
        const unsigned gx = (w + 255) / 256, row_groups = (h + 3) / 4;
        const unsigned gy_cap = gx >= 2048 ? 1 : 2048 / gx;
        const unsigned gy = row_groups < gy_cap ? row_groups : gy_cap;
        hipLaunchKernelGGL(kernel, dim3(gx, gy), dim3(256), 0, s0.stream, ptr[0], stride[0], ptr[1], stride[1], ptr[2], stride[2], w, h, o);
        const hipError_t e = hipGetLastError();
        if(e != hipSuccess) { return j2p_fail(J2P_EDEVICE, "planes_to_tensor: %s", hipGetErrorString(e)); }
        return J2P_OK;
}

int j2p_device_of_pointer(const void *p, int *device)
{
        hipPointerAttribute_t attr;
        memset(&attr, 0, sizeof(attr));
        if(hipPointerGetAttributes(&attr, p) != hipSuccess) {
                (void)hipGetLastError();                 // (plain host memory is an error to some runtimes, "unregistered" to others)
                return J2P_EINVAL;
        }
        if(attr.type != hipMemoryTypeDevice || attr.isManaged) { return J2P_EINVAL; }
        *device = attr.device;
        return J2P_OK;
}

int j2p_memory_of_pointer(const void *p, int *device)
{
        hipPointerAttribute_t attr;
        memset(&attr, 0, sizeof(attr));
        if(hipPointerGetAttributes(&attr, p) != hipSuccess) {
                (void)hipGetLastError();                 // (plain host memory is an error to some runtimes, "unregistered" to others)
                return J2P_MEMORY_HOST;
        }
        if(attr.isManaged || attr.type == hipMemoryTypeManaged) { return J2P_MEMORY_OTHER; }
        if(attr.type == hipMemoryTypeDevice) {
                *device = attr.device;
                return J2P_MEMORY_DEVICE;
        }
        return attr.type == hipMemoryTypeHost || attr.type == hipMemoryTypeUnregistered ? J2P_MEMORY_HOST : J2P_MEMORY_OTHER;
}

int j2p_planes_to_tensor(const j2p_plane_ref planes[], unsigned nplane, unsigned w, unsigned h, const j2p_tensor *out)
{
        return tensor_rows(planes, nplane, true, w, 0, h, out);
}

int j2p_planes_rows_to_tensor(const j2p_plane_ref planes[], unsigned nplane, unsigned w, unsigned row_begin, unsigned row_end,
                              const j2p_tensor *out)
{
        return tensor_rows(planes, nplane, false, w, row_begin, row_end, out);
}

// ---- resized tensor output: k_to_tensor_resized ----
using ResizedKernel = void (*)(const float *, unsigned, const float *, unsigned, const float *, unsigned, ResizeGeom, TensorOut);
#define J2P_RESIZED_ROW(NPLANE) \
        {k_to_tensor_resized<NPLANE, kDtypeU8>, k_to_tensor_resized<NPLANE, kDtypeF16>, k_to_tensor_resized<NPLANE, kDtypeBF16>, k_to_tensor_resized<NPLANE, kDtypeF32>}
static const ResizedKernel kResizedKernels[2][4] = {J2P_RESIZED_ROW(3), J2P_RESIZED_ROW(1)};            // [three planes / one][dtype]
#undef J2P_RESIZED_ROW

// The tile of k_to_tensor_resized — output columns and consecutive output rows per wavefront — the only place that knows the
// rule.  256 columns (64 lanes x 4) make a wavefront's source segment at least as long as k_to_tensor's 256 pixels at any
// ratio; but a small output of a large image has few such tiles and every one of them a long footprint, so the tile is
// halved while the chip (256 CUs x 4 SIMDs) would get fewer than two wavefronts per SIMD — not below 32 columns: the lanes
// beyond the tile's columns only load and convert, they walk no taps.  Rows: a wavefront that owns several consecutive
// output rows reads and converts the source row that two of them share once instead of twice (at ratios just above 1
// that is every row) and spreads its set-up over them; up to 8, as long as about four wavefronts per SIMD remain.
// Same bits for every tile: a column's sums do not depend on which lane or wavefront forms them.
static void resize_tile(unsigned out_w, unsigned out_h, unsigned *lanes, unsigned *slots, unsigned *rows)
{
        unsigned tile = 64 * kResizeSlots;
        while(tile > 32 && (unsigned long long)((out_w + tile - 1) / tile) * out_h < 2048) { tile /= 2; }
        *lanes = tile < 64 ? tile : 64;
        *slots = tile / *lanes;
        const unsigned long long tiles = (out_w + tile - 1) / tile;
        unsigned r = 8;
        while(r > 1 && tiles * ((out_h + r - 1) / r) < 4096) { r /= 2; }
        while(((out_h + r - 1) / r + 3) / 4 > 65535) { r *= 2; }                // (what a grid's y dimension may be)
        *rows = r;
}

int j2p_planes_to_tensor_resized(const j2p_plane_ref planes[], unsigned nplane, unsigned w, unsigned h, const j2p_resize *r,
                                 const j2p_tensor *out)
{
        if(!planes || !out) { return j2p_fail(J2P_EINVAL, "NULL argument"); }
        if(const char *why = j2p_resize_error(r, w, h)) { return j2p_fail(J2P_EINVAL, "to_tensor: %s", why); }
        const float *ptr[3];
        unsigned stride[3];
        TensorOut o;
        j2p_solver_view s0;
        if(const int rc = tensor_resolve(planes, nplane, true, w, 0, h, out, ptr, stride, o, s0); rc != J2P_OK) { return rc; }
        DeviceGuard guard(s0.device);
        ResizeGeom g;
        g.box_x = r->box_x;
        g.box_y = r->box_y;
        const bool rx = r->out_w != r->box_w, ry = r->out_h != r->box_h;        // an axis that is not resized: one tap of weight 1
        g.tap_bw = rx ? r->box_w : 1;
        g.tap_ow = rx ? r->out_w : 1;
        g.tap_bh = ry ? r->box_h : 1;
        g.tap_oh = ry ? r->out_h : 1;
        g.out_w = r->out_w;
        g.out_h = r->out_h;
        g.div_x = rx ? (float)r->box_w : 0.f;
        g.div_y = ry ? (float)r->box_h : 0.f;
        resize_tile(r->out_w, r->out_h, &g.lanes, &g.slots, &g.rows);
        // what lets the kernel step from one column's taps to the next without dividing
        g.qx = g.tap_bw / g.tap_ow;
        g.rx = g.tap_bw % g.tap_ow;
        g.qy = g.tap_bh / g.tap_oh;
        g.ry = g.tap_bh % g.tap_oh;
        g.qlanes = (unsigned)((unsigned long long)g.lanes * g.tap_bw / g.tap_ow);
        g.rlanes = (unsigned)((unsigned long long)g.lanes * g.tap_bw % g.tap_ow);
        // a workgroup: 4 wavefronts, one above the other, of one tile
        const unsigned tile = g.lanes * g.slots, gx = (r->out_w + tile - 1) / tile, gy = ((r->out_h + g.rows - 1) / g.rows + 3) / 4;
        hipLaunchKernelGGL(kResizedKernels[nplane == 3 ? 0 : 1][out->dtype], dim3(gx, gy), dim3(256), 0, s0.stream, ptr[0], stride[0], ptr[1],
                           stride[1], ptr[2], stride[2], g, o);
        const hipError_t e = hipGetLastError();
        if(e != hipSuccess) { return j2p_fail(J2P_EDEVICE, "planes_to_tensor_resized: %s", hipGetErrorString(e)); }
        return J2P_OK;
}

// ---- filtered tensor output: k_filter_taps, k_to_tensor_filtered ----
static_assert(J2P_FILTER_TRIANGLE == kFilterTriangle && J2P_FILTER_CUBIC == kFilterCubic, "the kernels' filter codes are the header's");
using FilteredKernel = void (*)(const float *, unsigned, const float *, unsigned, const float *, unsigned, FilterGeom, TensorOut);
#define J2P_FILTERED_ROW(NPLANE) \
        {k_to_tensor_filtered<NPLANE, kDtypeU8>, k_to_tensor_filtered<NPLANE, kDtypeF16>, k_to_tensor_filtered<NPLANE, kDtypeBF16>, k_to_tensor_filtered<NPLANE, kDtypeF32>}
static const FilteredKernel kFilteredKernels[2][4] = {J2P_FILTERED_ROW(3), J2P_FILTERED_ROW(1)};          // [three planes / one][dtype]
#undef J2P_FILTERED_ROW

// Weights per output index in the scratch: ceil(2 * sup) + 2, with sup as filter_taps forms it.  A window has at most
// trunc(c + sup + 0.5) - trunc(c - sup + 0.5) <= 2 * sup + 1 taps (plus what rounding c -+ sup adds: far below 1), so
// ceil(2 * sup) + 1 hold every count and one more is spare.  An axis that is not resized has one tap.
static unsigned filter_stride(int filter, unsigned box, unsigned out)
{
        if(out == box) { return 1; }
        const double R = filter == kFilterCubic ? 2. : 1.;
        const double scale = (double)box / (double)out;
        const double sup = R * (scale > 1. ? scale : 1.);
        const unsigned long long whole = (unsigned long long)(2. * sup);
        return (unsigned)(whole + ((double)whole < 2. * sup ? 1 : 0) + 2);
}

int j2p_debug_filter_taps(int filter, unsigned box, unsigned out, unsigned X, unsigned *first, unsigned *count, float *weights,
                          unsigned capacity)
{
        if(!first || !count || (!weights && capacity)) { return j2p_fail(J2P_EINVAL, "NULL argument"); }
        if(filter != J2P_FILTER_TRIANGLE && filter != J2P_FILTER_CUBIC) { return j2p_fail(J2P_EINVAL, "filter_taps: unknown filter %d", filter); }
        if(box == 0 || out == 0 || X >= out) { return j2p_fail(J2P_EINVAL, "filter_taps: box %u, out %u, index %u", box, out, X); }
        filter_taps(filter, box, out, X, first, count, capacity, [&](unsigned t, float f) { weights[t] = f; });
        if(*count > capacity) { return j2p_fail(J2P_EINVAL, "filter_taps: %u taps, room for %u", *count, capacity); }
        return J2P_OK;
}

// The tile of k_to_tensor_filtered: 256 columns x kFilterRows rows per wavefront where that still gives the chip (256 CUs x
// 4 SIMDs) two wavefronts per SIMD.  Where it does not, columns go first, down to 64: a narrower tile converts 2R * fs more
// source columns per tile, a few percent, while every output row a wavefront gives up makes it convert and walk the source
// rows it shared with its neighbours (2R * fs of them) once more — (rows - 1 + 2R) / rows conversions per source row, 1.25
// for the triangle at 4 rows and 2 at one.  Then rows, and last 32 columns, where half the lanes walk no taps (more
// wavefronts still beat fuller ones there: j2p_output_kernels.hip.h).  Same bits for every tile.
static void filter_tile(unsigned out_w, unsigned out_h, unsigned *lanes, unsigned *slots, unsigned *rows)
{
        unsigned tile = 64 * kResizeSlots, r = kFilterRows;
        const auto few = [&] { return (unsigned long long)((out_w + tile - 1) / tile) * ((out_h + r - 1) / r) < 2048; };
        while(tile > 64 && few()) { tile /= 2; }
        while(r > 1 && few()) { r /= 2; }
        if(few()) { tile = 32; }
        *lanes = tile < 64 ? tile : 64;
        *slots = tile / *lanes;
        *rows = r;                              // (out_h <= 65536: the grid's y dimension is at most 16384)
}

// What one filtered output needs, from its spec alone (host arithmetic: the single call, the call of several outputs and the
// work-map hooks all plan with this).  Its scratch, in 32-bit words:
// [first_x, count_x: out_w ints each][first_y, count_y: out_h][wx: out_w * stride_x floats][wy: out_h * stride_y]
struct OutputPlan {
        unsigned stride_x, stride_y;    // weights per output column / row
        size_t words;
        unsigned lanes, slots, rows;    // the tile
        unsigned gx, gy;                // its own grid: tile columns x row groups; a workgroup is 4 wavefronts, one above the other, of one tile
};
static OutputPlan plan_output(const j2p_resample &r)
{
        OutputPlan p;
        p.stride_x = filter_stride(r.filter, r.box_w, r.out_w);
        p.stride_y = filter_stride(r.filter, r.box_h, r.out_h);
        p.words = 2 * ((size_t)r.out_w + r.out_h) + (size_t)r.out_w * p.stride_x + (size_t)r.out_h * p.stride_y;
        filter_tile(r.out_w, r.out_h, &p.lanes, &p.slots, &p.rows);
        const unsigned tile = p.lanes * p.slots;
        p.gx = (r.out_w + tile - 1) / tile;
        p.gy = ((r.out_h + p.rows - 1) / p.rows + 3) / 4;
        return p;
}
// the arguments of both kernels for an output whose scratch starts at `ints`
static void bind_output(const j2p_resample &r, const OutputPlan &p, int *ints, FilterAxis &ax, FilterAxis &ay, FilterGeom &g)
{
        ax.box = r.box_w;
        ax.out = r.out_w;
        ax.stride = p.stride_x;
        ay.box = r.box_h;
        ay.out = r.out_h;
        ay.stride = p.stride_y;
        ax.first = ints;
        ax.count = ints + ax.out;
        ay.first = ints + 2 * (size_t)ax.out;
        ay.count = ay.first + ay.out;
        ax.weights = reinterpret_cast<float *>(ay.count + ay.out);
        ay.weights = ax.weights + (size_t)ax.out * ax.stride;
        g.box_x = r.box_x;
        g.box_y = r.box_y;
        g.out_w = r.out_w;
        g.out_h = r.out_h;
        g.stride_x = ax.stride;
        g.stride_y = ay.stride;
        g.first_x = ax.first;
        g.count_x = ax.count;
        g.first_y = ay.first;
        g.count_y = ay.count;
        g.wx = ax.weights;
        g.wy = ay.weights;
        g.lanes = p.lanes;
        g.slots = p.slots;
        g.rows = p.rows;
}

int j2p_planes_to_tensor_resampled(const j2p_plane_ref planes[], unsigned nplane, unsigned w, unsigned h, const j2p_resample *r,
                                   const j2p_tensor *out)
{
        if(!planes || !out) { return j2p_fail(J2P_EINVAL, "NULL argument"); }
        if(const char *why = j2p_resample_error(r, w, h)) { return j2p_fail(J2P_EINVAL, "to_tensor: %s", why); }
        const float *ptr[3];
        unsigned stride[3];
        TensorOut o;
        j2p_solver_view s0;
        if(const int rc = tensor_resolve(planes, nplane, true, w, 0, h, out, ptr, stride, o, s0); rc != J2P_OK) { return rc; }
        DeviceGuard guard(s0.device);
        const OutputPlan p = plan_output(*r);
        void *scratch = nullptr;
        if(const int rc = j2p_solver_scratch(planes[0].solver, p.words * 4, &scratch); rc != J2P_OK) { return rc; }
        FilterAxis ax, ay;
        FilterGeom g;
        bind_output(*r, p, static_cast<int *>(scratch), ax, ay, g);
        const unsigned most = ax.out > ay.out ? ax.out : ay.out;
        hipLaunchKernelGGL(k_filter_taps, dim3((most + 255) / 256, 2), dim3(256), 0, s0.stream, r->filter, ax, ay);
        hipLaunchKernelGGL(kFilteredKernels[nplane == 3 ? 0 : 1][out->dtype], dim3(p.gx, p.gy), dim3(256), 0, s0.stream, ptr[0], stride[0], ptr[1],
                           stride[1], ptr[2], stride[2], g, o);
        const hipError_t e = hipGetLastError();
        if(e != hipSuccess) { return j2p_fail(J2P_EDEVICE, "planes_to_tensor_resampled: %s", hipGetErrorString(e)); }
        return J2P_OK;
}

// ---- several filtered outputs in one call: k_filter_taps_outputs, k_to_tensors_filtered ----
static_assert(J2P_MAX_OUTPUTS == kMaxOutputs, "the kernels' tables hold the header's number of outputs");
using FilteredOutputsKernel = void (*)(const float *, unsigned, const float *, unsigned, const float *, unsigned, FilterOutputs);
#define J2P_FILTERED_ROW(NPLANE) \
        {k_to_tensors_filtered<NPLANE, kDtypeU8>, k_to_tensors_filtered<NPLANE, kDtypeF16>, k_to_tensors_filtered<NPLANE, kDtypeBF16>, k_to_tensors_filtered<NPLANE, kDtypeF32>}
static const FilteredOutputsKernel kFilteredOutputsKernels[2][4] = {J2P_FILTERED_ROW(3), J2P_FILTERED_ROW(1)};   // [three planes / one][dtype]
#undef J2P_FILTERED_ROW

// The work of a call of n outputs, from the specs and the dtypes alone: every output's plan as the single call makes it — the
// same tile: whether a tile chosen from the call's total does better has not been measured — its place in the scratch (one
// after the other: the size is the sum), and the sampling launches: one per dtype present, in ascending dtype code, each
// with its outputs in list order and the prefix table of their workgroups.
struct CallPlan {
        OutputPlan out[kMaxOutputs];
        size_t word0[kMaxOutputs], words;
        unsigned launch_of[kMaxOutputs];
        unsigned nlaunch;
        int dtype[4];
        unsigned count[4], member[4][kMaxOutputs], end[4][kMaxOutputs];
};
static void plan_call(unsigned n, const j2p_resample specs[], const int dtypes[], CallPlan &c)
{
        c.words = 0;
        for(unsigned i = 0; i < n; i++) {
                c.out[i] = plan_output(specs[i]);
                c.word0[i] = c.words;
                c.words += c.out[i].words;
        }
        c.nlaunch = 0;
        for(int d = J2P_DTYPE_U8; d <= J2P_DTYPE_F32; d++) {
                unsigned m = 0, workgroups = 0;
                for(unsigned i = 0; i < n; i++) {
                        if(dtypes[i] != d) { continue; }
                        workgroups += c.out[i].gx * c.out[i].gy;          // (16 outputs of at most 2^20 workgroups each)
                        c.member[c.nlaunch][m] = i;
                        c.end[c.nlaunch][m] = workgroups;
                        c.launch_of[i] = c.nlaunch;
                        m++;
                }
                if(m == 0) { continue; }
                c.dtype[c.nlaunch] = d;
                c.count[c.nlaunch] = m;
                c.nlaunch++;
        }
}

int j2p_planes_to_tensors_resampled(const j2p_plane_ref planes[], unsigned nplane, unsigned w, unsigned h, unsigned n, const j2p_output outs[])
{
        if(!planes || !outs) { return j2p_fail(J2P_EINVAL, "NULL argument"); }
        if(n == 0 || n > J2P_MAX_OUTPUTS) { return j2p_fail(J2P_EINVAL, "to_tensors: %u outputs (1..%d)", n, J2P_MAX_OUTPUTS); }
        if(n == 1) { return j2p_planes_to_tensor_resampled(planes, nplane, w, h, &outs[0].r, &outs[0].t); }
        // every check of every output, before anything is queued
        const float *ptr[3];
        unsigned stride[3];
        TensorOut o[kMaxOutputs];
        j2p_solver_view s0;
        for(unsigned i = 0; i < n; i++) {
                if(const char *why = j2p_resample_error(&outs[i].r, w, h)) { return j2p_fail(J2P_EINVAL, "to_tensors: output %u: %s", i, why); }
        }
        for(unsigned i = 0; i < n; i++) {
                if(const int rc = tensor_resolve(planes, nplane, true, w, 0, h, &outs[i].t, ptr, stride, o[i], s0); rc != J2P_OK) { return rc; }
        }
        DeviceGuard guard(s0.device);
        j2p_resample specs[kMaxOutputs];
        int dtypes[kMaxOutputs];
        for(unsigned i = 0; i < n; i++) {
                specs[i] = outs[i].r;
                dtypes[i] = outs[i].t.dtype;
        }
        CallPlan c;
        plan_call(n, specs, dtypes, c);
        void *scratch = nullptr;
        if(const int rc = j2p_solver_scratch(planes[0].solver, c.words * 4, &scratch); rc != J2P_OK) { return rc; }
        FilterAxes axes;
        FilterGeom g[kMaxOutputs];
        axes.n = 2 * n;
        unsigned tap_workgroups = 0;
        for(unsigned i = 0; i < n; i++) {
                bind_output(outs[i].r, c.out[i], static_cast<int *>(scratch) + c.word0[i], axes.axis[2 * i], axes.axis[2 * i + 1], g[i]);
                for(unsigned a = 2 * i; a < 2 * i + 2; a++) {
                        axes.filter[a] = outs[i].r.filter;
                        tap_workgroups += (axes.axis[a].out + 255) / 256;
                        axes.end[a] = tap_workgroups;
                }
        }
        hipLaunchKernelGGL(k_filter_taps_outputs, dim3(tap_workgroups), dim3(256), 0, s0.stream, axes);
        for(unsigned l = 0; l < c.nlaunch; l++) {
                FilterOutputs f;
                f.n = c.count[l];
                for(unsigned m = 0; m < f.n; m++) {
                        const unsigned i = c.member[l][m];
                        f.end[m] = c.end[l][m];
                        f.columns[m] = c.out[i].gx;
                        f.g[m] = g[i];
                        f.o[m] = o[i];
                }
                hipLaunchKernelGGL(kFilteredOutputsKernels[nplane == 3 ? 0 : 1][c.dtype[l]], dim3(f.end[f.n - 1]), dim3(256), 0, s0.stream, ptr[0],
                                   stride[0], ptr[1], stride[1], ptr[2], stride[2], f);
        }
        const hipError_t e = hipGetLastError();
        if(e != hipSuccess) { return j2p_fail(J2P_EDEVICE, "planes_to_tensors_resampled: %s", hipGetErrorString(e)); }
        return J2P_OK;
}

// what both hooks check: the specs as the call checks them, and the dtype codes
static int debug_outputs_check(unsigned w, unsigned h, unsigned n, const j2p_resample specs[], const int dtypes[])
{
        if(!specs || !dtypes) { return j2p_fail(J2P_EINVAL, "NULL argument"); }
        if(n == 0 || n > J2P_MAX_OUTPUTS) { return j2p_fail(J2P_EINVAL, "to_tensors: %u outputs (1..%d)", n, J2P_MAX_OUTPUTS); }
        for(unsigned i = 0; i < n; i++) {
                if(const char *why = j2p_resample_error(&specs[i], w, h)) { return j2p_fail(J2P_EINVAL, "to_tensors: output %u: %s", i, why); }
                if(dtypes[i] < J2P_DTYPE_U8 || dtypes[i] > J2P_DTYPE_F32) { return j2p_fail(J2P_EINVAL, "to_tensors: output %u: unknown dtype %d", i, dtypes[i]); }
        }
        return J2P_OK;
}

int j2p_debug_outputs_plan(unsigned w, unsigned h, unsigned n, const j2p_resample specs[], const int dtypes[], unsigned tiles[], unsigned grids[],
                           unsigned launch_of[], unsigned *nlaunch, int launch_dtype[4], unsigned launch_workgroups[4])
{
        if(!tiles || !grids || !launch_of || !nlaunch || !launch_dtype || !launch_workgroups) { return j2p_fail(J2P_EINVAL, "NULL argument"); }
        if(const int rc = debug_outputs_check(w, h, n, specs, dtypes); rc != J2P_OK) { return rc; }
        CallPlan c;
        plan_call(n, specs, dtypes, c);
        for(unsigned i = 0; i < n; i++) {
                tiles[3 * i] = c.out[i].lanes;
                tiles[3 * i + 1] = c.out[i].slots;
                tiles[3 * i + 2] = c.out[i].rows;
                grids[2 * i] = c.out[i].gx;
                grids[2 * i + 1] = c.out[i].gy;
                launch_of[i] = c.launch_of[i];
        }
        *nlaunch = c.nlaunch;
        for(unsigned l = 0; l < c.nlaunch; l++) {
                launch_dtype[l] = c.dtype[l];
                launch_workgroups[l] = c.end[l][c.count[l] - 1];
        }
        return J2P_OK;
}

int j2p_debug_outputs_workgroups(unsigned w, unsigned h, unsigned n, const j2p_resample specs[], const int dtypes[], unsigned launch,
                                 unsigned first, unsigned count, unsigned map[])
{
        if(!map && count) { return j2p_fail(J2P_EINVAL, "NULL argument"); }
        if(const int rc = debug_outputs_check(w, h, n, specs, dtypes); rc != J2P_OK) { return rc; }
        CallPlan c;
        plan_call(n, specs, dtypes, c);
        if(launch >= c.nlaunch) { return j2p_fail(J2P_EINVAL, "to_tensors: launch %u of %u", launch, c.nlaunch); }
        const unsigned total = c.end[launch][c.count[launch] - 1];
        if(first > total || count > total - first) { return j2p_fail(J2P_EINVAL, "to_tensors: workgroups [%u, %u + %u) of %u", first, first, count, total); }
        for(unsigned k = 0; k < count; k++) {
                // what k_to_tensors_filtered's workgroup first + k does with its table
                unsigned local;
                const unsigned m = output_of_workgroup(c.end[launch], c.count[launch], first + k, &local);
                const unsigned columns = c.out[c.member[launch][m]].gx, by = local / columns;
                map[3 * k] = c.member[launch][m];
                map[3 * k + 1] = local - by * columns;
                map[3 * k + 2] = by;
        }
        return J2P_OK;
}

// what quantise_check found: enough to queue the kernel
struct QuantiseLaunch {
        j2p_solver_view s;
        const float *src;               // the first canvas row of block row r0
        unsigned rows;                  // canvas rows from there to the end of what the solver holds
        QuantSteps steps;
};
// block rows [r0, r1) x blocks_w blocks of one (solver, channel) pair as quantised coefficients of the plane at
// 1/sub_w x 1/sub_h of its resolution (k_quantise_blocks<sub_w, sub_h>): output block row r covers canvas rows
// [8 * sub_h * r, 8 * sub_h * (r + 1)).  `whole`: called as a whole-canvas form, which band solvers refuse.
// In three steps, so that the JPEG file's coder can check every plane before it queues anything and keep the coefficients
// on the device: quantise_check (arguments and state), quantise_queue (the launch), quantise_rows (both, and the download).
static int quantise_check(const j2p_plane_ref *plane, bool whole, unsigned sub_w, unsigned sub_h, unsigned blocks_w, unsigned r0,
                          unsigned r1, const uint16_t quant_table[64], QuantiseLaunch &q)
{
        if(!plane || !quant_table) { return j2p_fail(J2P_EINVAL, "NULL argument"); }
        if(blocks_w == 0 || r0 >= r1) { return j2p_fail(J2P_EINVAL, whole ? "empty image" : "empty row range"); }
        const j2p_solver_view s = plane->solver ? j2p_solver_view_of(plane->solver) : j2p_solver_view{};
        if(whole && plane->solver && !s.whole) {
                return j2p_fail(J2P_ESTATE, "to_coefficients needs a whole-canvas solver (bands: the j2p_planes_rows_to_coefficients forms)");
        }
        if(sub_w < 1 || sub_w > 2 || sub_h < 1 || sub_h > 2) {
                return j2p_fail(J2P_EINVAL, "to_coefficients: sampling factors %ux%u (1 and 2 are supported)", sub_w, sub_h);
        }
        if(!plane->solver || plane->channel >= s.nch) { return j2p_fail(J2P_EINVAL, "plane 0: bad solver/channel"); }
        QuantSteps &steps = q.steps;
        for(int j = 0; j < 64; j++) {
                if(quant_table[j] == 0) { return j2p_fail(J2P_EINVAL, "to_coefficients: quantisation table entry %d is zero", j); }
                steps.q[j] = (float)quant_table[j];
        }
        // One rule for every sampling: every block starts inside the solver's rows and columns, and rows beyond the band are
        // replicated only where the band ends with the canvas (a band that is not the last ends on a multiple of 16).  For 1x1
        // that is "the whole grid inside": W, the band's rows and every block's start are multiples of 8, so a block that starts
        // inside ends inside.
        const unsigned long long row_end = (unsigned long long)s.row0 + s.rows, step_y = 8ull * sub_h;
        if(8ull * sub_w * (blocks_w - 1) >= s.W || step_y * r0 < s.row0 || step_y * (r1 - 1) >= row_end ||
           (step_y * r1 > row_end && row_end != s.H)) {
                return j2p_fail(J2P_EINVAL, "to_coefficients: block rows [%u,%u) x %u blocks of %ux%u-pixel samples are not inside the solver's rows "
                            "[%u,%u) x %u columns (every block must start there; only the canvas's last rows and columns are replicated)",
                            r0, r1, blocks_w, sub_w, sub_h, s.row0, s.row0 + s.rows, s.W);
        }
        if(s.mid_iteration) { return j2p_fail(J2P_ESTATE, "to_coefficients between the two phases of an iteration"); }
        const unsigned first = (unsigned)(step_y * r0);
        const float *src = nullptr;
        if(const int rc = j2p_solver_row(plane->solver, plane->channel, first, &src); rc != J2P_OK) { return rc; }
        q.s = s;
        q.src = src;
        q.rows = (unsigned)(row_end - first);
        return J2P_OK;
}
// block rows [r0, r1) x blocks_w blocks of what quantise_check accepted into device memory `dout`, queued on `stream`
static void quantise_queue(const QuantiseLaunch &q, unsigned sub_w, unsigned sub_h, unsigned blocks_w, unsigned r0, unsigned r1, hipStream_t stream,
                           int16_t *dout)
{
        const unsigned long long groups = (unsigned long long)((blocks_w + 7) / 8) * (r1 - r0);
        const auto kernel = sub_w == 2 ? (sub_h == 2 ? k_quantise_blocks<2, 2> : k_quantise_blocks<2, 1>)
                                       : (sub_h == 2 ? k_quantise_blocks<1, 2> : k_quantise_blocks<1, 1>);
        hipLaunchKernelGGL(kernel, dim3((unsigned)((groups + 3) / 4)), dim3(256), 0, stream, q.src, q.s.W, q.rows, blocks_w, r1 - r0, q.steps, dout);
}
static int quantise_rows(const j2p_plane_ref *plane, bool whole, unsigned sub_w, unsigned sub_h, unsigned blocks_w, unsigned r0,
                         unsigned r1, const uint16_t quant_table[64], int16_t *out_host)
{
        if(!out_host) { return j2p_fail(J2P_EINVAL, "NULL argument"); }
        QuantiseLaunch q;
        if(const int rc = quantise_check(plane, whole, sub_w, sub_h, blocks_w, r0, r1, quant_table, q); rc != J2P_OK) { return rc; }
        const j2p_solver_view &s = q.s;
        DeviceGuard guard(s.device);
        const size_t bytes = (size_t)blocks_w * (r1 - r0) * 64 * sizeof(int16_t);
        void *dout = nullptr;
        size_t dout_bytes = 0;
        HIP_TRY(j2p_pool_take(s.device, bytes, &dout, &dout_bytes));
        quantise_queue(q, sub_w, sub_h, blocks_w, r0, r1, s.stream, static_cast<int16_t *>(dout));
        hipError_t e = hipGetLastError();
        if(e == hipSuccess) { e = hipMemcpyAsync(out_host, dout, bytes, hipMemcpyDeviceToHost, s.stream); }
        if(e == hipSuccess) { e = hipStreamSynchronize(s.stream); }
        j2p_pool_give(s.device, dout, dout_bytes);
        if(e != hipSuccess) { return j2p_fail(J2P_EDEVICE, "planes_to_coefficients: %s", hipGetErrorString(e)); }
        return J2P_OK;
}

int j2p_planes_to_coefficients(const j2p_plane_ref *plane, unsigned blocks_w, unsigned blocks_h, const uint16_t quant_table[64],
                               int16_t *out_host)
{
        return quantise_rows(plane, true, 1, 1, blocks_w, 0, blocks_h, quant_table, out_host);
}

int j2p_planes_rows_to_coefficients(const j2p_plane_ref *plane, unsigned blocks_w, unsigned block_row_begin, unsigned block_row_end,
                                    const uint16_t quant_table[64], int16_t *out_host)
{
        return quantise_rows(plane, false, 1, 1, blocks_w, block_row_begin, block_row_end, quant_table, out_host);
}

int j2p_planes_to_coefficients_sub(const j2p_plane_ref *plane, unsigned sub_w, unsigned sub_h, unsigned blocks_w, unsigned blocks_h,
                                   const uint16_t quant_table[64], int16_t *out_host)
{
        return quantise_rows(plane, true, sub_w, sub_h, blocks_w, 0, blocks_h, quant_table, out_host);
}

int j2p_planes_rows_to_coefficients_sub(const j2p_plane_ref *plane, unsigned sub_w, unsigned sub_h, unsigned blocks_w,
                                        unsigned block_row_begin, unsigned block_row_end, const uint16_t quant_table[64], int16_t *out_host)
{
        return quantise_rows(plane, false, sub_w, sub_h, blocks_w, block_row_begin, block_row_end, quant_table, out_host);
}

}  // extern "C"

// ---- the JPEG file: k_entropy_lengths, k_scan_*, k_entropy_pack, k_stuff_count, k_stuff_copy ----
namespace {

// Annex K.3 of the JPEG standard, as include/jpeg2png_amd.h states them: [0] the tables of component 0, [1] of the others
const uint8_t kDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
const uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t kAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
const uint8_t kAcVals[2][162] = {
        {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
         0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
         0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
         0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
         0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
         0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
         0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
         0xfa},
        {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
         0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
         0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
         0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
         0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
         0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
         0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
         0xfa}};
// natural index of zigzag position k (the kernels' kZigzagNatural)
const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                             35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// the codes of one table, by symbol: in order of length, consecutive within a length, doubled from one length to the next
void huffman_codes(const uint8_t bits[16], const uint8_t *vals, unsigned *by_symbol)
{
        unsigned code = 0, k = 0;
        for(unsigned length = 1; length <= 16; length++) {
                for(unsigned i = 0; i < bits[length - 1]; i++) { by_symbol[vals[k++]] = (length << 16) | code++; }
                code <<= 1;
        }
}
const HuffCodes &huffman_tables()
{
        static const HuffCodes tables = [] {
                HuffCodes h;
                memset(&h, 0, sizeof(h));
                for(int t = 0; t < 2; t++) {
                        huffman_codes(kDcBits[t], kDcVals, h.dc[t]);
                        huffman_codes(kAcBits[t], kAcVals[t], h.ac[t]);
                }
                return h;
        }();
        return tables;
}

// everything in front of the entropy-coded data; at most 623 bytes.  Returns their number.
constexpr size_t kJpegHeaderMax = 640;
size_t jpeg_header(const j2p_jpeg &spec, unsigned ncomp, uint8_t *out)
{
        uint8_t *p = out;
        const auto segment = [&](uint8_t marker, size_t payload) {
                *p++ = 0xff;
                *p++ = marker;
                *p++ = (uint8_t)((payload + 2) >> 8);
                *p++ = (uint8_t)(payload + 2);
        };
        *p++ = 0xff;
        *p++ = 0xd8;
        static const uint8_t jfif[14] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
        segment(0xe0, sizeof(jfif));
        memcpy(p, jfif, sizeof(jfif));
        p += sizeof(jfif);
        for(unsigned t = 0; t < (ncomp == 3 ? 2u : 1u); t++) {
                segment(0xdb, 65);
                *p++ = (uint8_t)t;
                for(int k = 0; k < 64; k++) { *p++ = (uint8_t)spec.quant[t][kZigzag[k]]; }
        }
        segment(0xc0, 6 + 3 * ncomp);
        *p++ = 8;
        *p++ = (uint8_t)(spec.height >> 8);
        *p++ = (uint8_t)spec.height;
        *p++ = (uint8_t)(spec.width >> 8);
        *p++ = (uint8_t)spec.width;
        *p++ = (uint8_t)ncomp;
        for(unsigned c = 0; c < ncomp; c++) {
                *p++ = (uint8_t)(c + 1);
                *p++ = c == 0 && ncomp == 3 ? (uint8_t)((spec.sub_w << 4) | spec.sub_h) : 0x11;
                *p++ = c ? 1 : 0;
        }
        for(unsigned t = 0; t < (ncomp == 3 ? 2u : 1u); t++) {
                segment(0xc4, 1 + 16 + 12);
                *p++ = (uint8_t)t;
                memcpy(p, kDcBits[t], 16);
                memcpy(p + 16, kDcVals, 12);
                p += 28;
                segment(0xc4, 1 + 16 + 162);
                *p++ = (uint8_t)(0x10 | t);
                memcpy(p, kAcBits[t], 16);
                memcpy(p + 16, kAcVals[t], 162);
                p += 178;
        }
        segment(0xda, 1 + 2 * ncomp + 3);
        *p++ = (uint8_t)ncomp;
        for(unsigned c = 0; c < ncomp; c++) {
                *p++ = (uint8_t)(c + 1);
                *p++ = c ? 0x11 : 0x00;
        }
        *p++ = 0;
        *p++ = 0x3f;
        *p++ = 0;
        return (size_t)(p - out);
}

// the component grids of a spec that j2p_jpeg_error accepted, and the scan's geometry but for the coefficients' addresses
ScanGeom scan_geometry(const j2p_jpeg &spec, unsigned ncomp)
{
        ScanGeom g;
        memset(&g, 0, sizeof(g));
        g.ncomp = ncomp;
        g.sub_w = ncomp == 3 ? spec.sub_w : 1;
        g.sub_h = ncomp == 3 ? spec.sub_h : 1;
        g.bw[0] = (spec.width + 7) / 8;
        g.bh[0] = (spec.height + 7) / 8;
        g.mcus_w = (g.bw[0] + g.sub_w - 1) / g.sub_w;
        const unsigned mcus_h = (g.bh[0] + g.sub_h - 1) / g.sub_h;
        for(unsigned c = 1; c < ncomp; c++) {
                g.bw[c] = g.mcus_w;
                g.bh[c] = mcus_h;
        }
        g.per_mcu = ncomp == 3 ? g.sub_w * g.sub_h + 2 : 1;
        g.nslots = ncomp == 3 ? g.mcus_w * mcus_h * g.per_mcu : g.bw[0] * g.bh[0];       // (at most 6 * 8192^2 / 4)
        return g;
}

size_t round_up(size_t v, size_t to) { return (v + to - 1) / to * to; }

// an exclusive sum of n counts on the stream: in -> out, sums: ceil(n / kScanTile) + 1 words, the last the total
void queue_scan(hipStream_t stream, const unsigned *in, unsigned n, unsigned long long *sums, unsigned long long *out)
{
        const unsigned ntiles = (n + kScanTile - 1) / kScanTile;
        hipLaunchKernelGGL(k_scan_sums, dim3(ntiles), dim3(256), 0, stream, in, n, sums);
        hipLaunchKernelGGL(k_scan_tiles, dim3(1), dim3(256), 0, stream, sums, ntiles);
        hipLaunchKernelGGL(k_scan_apply, dim3(ntiles), dim3(256), 0, stream, in, n, static_cast<const unsigned long long *>(sums), out);
}

// The coder.  memory(bytes, &p, &moved): one block of device memory of at least that size which stays the same block while it
// is large enough and is ANOTHER block (moved), contents lost, once it has to grow (j2p_solver_scratch); fill(stream, coef): queues what
// leaves component c's coefficients at coef[c].  The block's layout, each part aligned to 256 bytes:
//   [coefficients per component][len: nslots u32][off: nslots u64][sums: tiles + 1 u64]              known from the spec
//   [stage: the stream, ceil(bits / 32) + 1 words][count: chunks u32][ffoff: chunks u64][sums]      known once the bits are
//   [out: the stuffed bytes]                                                                        known once the FFs are
// so the two totals are read back (8 bytes each, a wait each) and the block is asked for three times, the first two times
// with a guess for what is not known yet; when it moved, what had been computed is computed again.  A second image of the
// same size or smaller finds the block large enough at once.
template <typename Memory, typename Fill>
int encode_scan(hipStream_t stream, const j2p_jpeg &spec, unsigned ncomp, Memory memory, Fill fill, uint8_t *out_host, size_t capacity,
                size_t *size)
{
        ScanGeom g = scan_geometry(spec, ncomp);
        const HuffCodes &codes = huffman_tables();
        const unsigned nslots = g.nslots, slot_tiles = (nslots + kScanTile - 1) / kScanTile;
        size_t coef_at[3], fixed = 0;
        for(unsigned c = 0; c < ncomp; c++) {
                coef_at[c] = fixed;
                fixed += round_up((size_t)g.bw[c] * g.bh[c] * 64 * sizeof(int16_t), 256);
        }
        const size_t coef_bytes = fixed;
        const size_t len_at = fixed, off_at = len_at + round_up((size_t)nslots * 4, 256), sums_at = off_at + round_up((size_t)nslots * 8, 256);
        fixed = sums_at + round_up(((size_t)slot_tiles + 1) * 8, 256);
        char *base = nullptr;
        const auto take = [&](size_t bytes, bool *moved) {
                void *p = nullptr;
                if(const int rc = memory(bytes, &p, moved); rc != J2P_OK) { return rc; }
                base = static_cast<char *>(p);
                return (int)J2P_OK;
        };
        const auto at = [&](size_t offset) { return base + offset; };
        // from the coefficients to the bit offsets
        const auto lengths = [&] {
                int16_t *coef[3] = {nullptr, nullptr, nullptr};
                for(unsigned c = 0; c < ncomp; c++) {
                        coef[c] = reinterpret_cast<int16_t *>(at(coef_at[c]));
                        g.coef[c] = coef[c];
                }
                fill(stream, coef);
                const unsigned per_workgroup = 4 * kEntropyIters;
                hipLaunchKernelGGL(k_entropy_lengths, dim3((nslots + per_workgroup - 1) / per_workgroup), dim3(256), 0, stream, g, codes,
                                   reinterpret_cast<unsigned *>(at(len_at)));
                queue_scan(stream, reinterpret_cast<unsigned *>(at(len_at)), nslots, reinterpret_cast<unsigned long long *>(at(sums_at)),
                           reinterpret_cast<unsigned long long *>(at(off_at)));
        };
        bool moved = false;
        if(const int rc = take(fixed + coef_bytes / 4, &moved); rc != J2P_OK) { return rc; }     // (a file is rarely an eighth of its coefficients)
        lengths();
        unsigned long long bits = 0;
        HIP_TRY(hipMemcpyAsync(&bits, at(sums_at) + (size_t)slot_tiles * 8, 8, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        const size_t nbytes = (size_t)((bits + 7) / 8), stage_words = (size_t)((bits + 31) / 32) + 1;
        const unsigned nchunks = (unsigned)((nbytes + kStuffChunk - 1) / kStuffChunk), chunk_tiles = (nchunks + kScanTile - 1) / kScanTile;
        const size_t stage_at = fixed, count_at = stage_at + round_up(stage_words * 4, 256), ffoff_at = count_at + round_up((size_t)nchunks * 4, 256);
        const size_t ffsums_at = ffoff_at + round_up((size_t)nchunks * 8, 256), out_at = ffsums_at + round_up(((size_t)chunk_tiles + 1) * 8, 256);
        // from the bit offsets to the stream and where its FF bytes are
        const auto pack = [&] {
                (void)hipMemsetAsync(at(stage_at), 0, stage_words * 4, stream);
                const unsigned per_workgroup = 4 * kEntropyIters;
                hipLaunchKernelGGL(k_entropy_pack, dim3((nslots + per_workgroup - 1) / per_workgroup), dim3(256), 0, stream, g, codes,
                                   reinterpret_cast<const unsigned long long *>(at(off_at)), reinterpret_cast<unsigned *>(at(stage_at)));
                hipLaunchKernelGGL(k_stuff_count, dim3((nchunks + 3) / 4), dim3(256), 0, stream, reinterpret_cast<const unsigned *>(at(stage_at)), nbytes,
                                   nchunks, reinterpret_cast<unsigned *>(at(count_at)));
                queue_scan(stream, reinterpret_cast<unsigned *>(at(count_at)), nchunks, reinterpret_cast<unsigned long long *>(at(ffsums_at)),
                           reinterpret_cast<unsigned long long *>(at(ffoff_at)));
        };
        if(const int rc = take(out_at + nbytes + nbytes / 16 + 256, &moved); rc != J2P_OK) { return rc; }
        if(moved) { lengths(); }
        pack();
        unsigned long long ffs = 0;
        HIP_TRY(hipMemcpyAsync(&ffs, at(ffsums_at) + (size_t)chunk_tiles * 8, 8, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        uint8_t header[kJpegHeaderMax];
        const size_t header_bytes = jpeg_header(spec, ncomp, header), data_bytes = nbytes + (size_t)ffs;
        *size = header_bytes + data_bytes + 2;
        if(capacity < *size || !out_host) { return j2p_fail(J2P_ESPACE, "jpeg: the file has %zu bytes, the buffer %zu", *size, out_host ? capacity : 0); }
        if(const int rc = take(out_at + data_bytes, &moved); rc != J2P_OK) { return rc; }
        if(moved) {
                lengths();
                pack();
        }
        hipLaunchKernelGGL(k_stuff_copy, dim3((nchunks + 3) / 4), dim3(256), 0, stream, reinterpret_cast<const unsigned *>(at(stage_at)), nbytes, nchunks,
                           reinterpret_cast<const unsigned long long *>(at(ffoff_at)), reinterpret_cast<uint8_t *>(at(out_at)));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(out_host + header_bytes, at(out_at), data_bytes, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        memcpy(out_host, header, header_bytes);
        out_host[header_bytes + data_bytes] = 0xff;
        out_host[header_bytes + data_bytes + 1] = 0xd9;
        return J2P_OK;
}

}  // namespace

extern "C" {

int j2p_planes_to_jpeg(const j2p_plane_ref planes[], unsigned nplane, const j2p_jpeg *spec, uint8_t *out_host, size_t capacity, size_t *size)
{
        if(!planes || !size) { return j2p_fail(J2P_EINVAL, "NULL argument"); }
        if(const char *why = j2p_jpeg_error(spec, nplane)) { return j2p_fail(J2P_EINVAL, "%s", why); }
        const ScanGeom g = scan_geometry(*spec, nplane);
        // every check of every plane, before anything is queued
        QuantiseLaunch q[3];
        for(unsigned c = 0; c < nplane; c++) {
                const unsigned sx = c ? g.sub_w : 1, sy = c ? g.sub_h : 1;
                if(const int rc = quantise_check(&planes[c], true, sx, sy, g.bw[c], 0, g.bh[c], spec->quant[c], q[c]); rc != J2P_OK) { return rc; }
                if(q[c].s.device != q[0].s.device) { return j2p_fail(J2P_EINVAL, "planes live on different devices"); }
        }
        DeviceGuard guard(q[0].s.device);
        const hipStream_t stream = q[0].s.stream;
        // everything is queued on planes[0].solver's stream: the other solvers' planes must be complete
        for(unsigned c = 1; c < nplane; c++) {
                if(planes[c].solver != planes[0].solver) { HIP_TRY(hipStreamSynchronize(q[c].s.stream)); }
        }
        j2p_solver *const owner = planes[0].solver;
        return encode_scan(
                stream, *spec, nplane, [&](size_t bytes, void **p, bool *moved) {
                        *moved = j2p_solver_scratch_bytes(owner) < bytes;
                        return j2p_solver_scratch(owner, bytes, p);
                },
                [&](hipStream_t st, int16_t *const coef[3]) {
                        for(unsigned c = 0; c < nplane; c++) { quantise_queue(q[c], c ? g.sub_w : 1, c ? g.sub_h : 1, g.bw[c], 0, g.bh[c], st, coef[c]); }
                },
                out_host, capacity, size);
}

int j2p_entropy_encode(int device, const j2p_jpeg *spec, const int16_t *const coef_host[3], unsigned ncomp, uint8_t *out_host, size_t capacity,
                       size_t *size)
{
        if(!coef_host || !size) { return j2p_fail(J2P_EINVAL, "NULL argument"); }
        if(const char *why = j2p_jpeg_error(spec, ncomp)) { return j2p_fail(J2P_EINVAL, "%s", why); }
        const ScanGeom g = scan_geometry(*spec, ncomp);
        size_t values[3] = {0, 0, 0};
        for(unsigned c = 0; c < ncomp; c++) {
                if(!coef_host[c]) { return j2p_fail(J2P_EINVAL, "jpeg: component %u has no coefficients", c); }
                values[c] = (size_t)g.bw[c] * g.bh[c] * 64;
                for(size_t i = 0; i < values[c]; i++) {
                        if(coef_host[c][i] < -1023 || coef_host[c][i] > 1023) {
                                return j2p_fail(J2P_EINVAL, "jpeg: component %u: coefficient %d (block %zu, index %zu) is outside [-1023, 1023]", c,
                                                coef_host[c][i], i / 64, i % 64);
                        }
                }
        }
        int have = 0;
        if(hipGetDeviceCount(&have) != hipSuccess || have <= 0) { return j2p_fail(J2P_EDEVICE, "no HIP device available"); }
        if(device < 0 || device >= have) { return j2p_fail(J2P_EINVAL, "device %d out of range (0..%d)", device, have - 1); }
        DeviceGuard guard(device);
        hipStream_t stream = nullptr;
        HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        // one pooled block that grows as the solvers' scratch does
        void *block = nullptr;
        size_t block_bytes = 0;
        const int rc = encode_scan(
                stream, *spec, ncomp,
                [&](size_t bytes, void **p, bool *moved) {
                        *moved = block_bytes < bytes;
                        if(block_bytes < bytes) {
                                HIP_TRY(hipStreamSynchronize(stream));
                                j2p_pool_give(device, block, block_bytes);
                                block = nullptr;
                                block_bytes = 0;
                                HIP_TRY(j2p_pool_take(device, bytes, &block, &block_bytes));
                        }
                        *p = block;
                        return (int)J2P_OK;
                },
                [&](hipStream_t st, int16_t *const coef[3]) {
                        for(unsigned c = 0; c < ncomp; c++) { (void)hipMemcpyAsync(coef[c], coef_host[c], values[c] * sizeof(int16_t), hipMemcpyHostToDevice, st); }
                },
                out_host, capacity, size);
        (void)hipStreamSynchronize(stream);
        j2p_pool_give(device, block, block_bytes);
        (void)hipStreamDestroy(stream);
        return rc;
}

}  // extern "C"

// ---- reading a JPEG file: k_unstuff_*, k_decode_* (j2p_decode_kernels.hip.h), the scans above ----
namespace {

DecodeTables decode_tables(const j2p_jpeg_parsed &p, unsigned S)
{
        DecodeTables t;
        memset(&t, 0, sizeof(t));
        for(int s = 0; s < 4; s++) {
                t.tab[s] = p.dc[s];
                t.tab[4 + s] = p.ac[s];
        }
        const j2p_jpeg_info &f = p.info;
        DecodeGeom &g = t.g;
        g.ncomp = f.ncomp;
        g.per_mcu = f.blocks_per_mcu;
        g.mcus_w = f.mcus_w;
        g.nmcus = f.mcus_w * f.mcus_h;
        g.ri = f.restart_interval ? f.restart_interval : g.nmcus;
        g.nint = f.intervals;
        g.nblocks = g.nmcus * g.per_mcu;
        g.S = S;
        unsigned blk = 0;
        for(unsigned c = 0; c < f.ncomp; c++) {
                g.bw[c] = f.comp[c].blocks_w;
                g.bh[c] = f.comp[c].blocks_h;
                g.hs[c] = f.ncomp == 1 ? 1 : f.comp[c].h_samp_factor;
                g.vs[c] = f.ncomp == 1 ? 1 : f.comp[c].v_samp_factor;
                g.first_blk[c] = blk;
                g.comp_base[c] = g.nmcus * blk;
                g.dc_tab[c] = f.comp[c].dc_slot;
                g.ac_tab[c] = f.comp[c].ac_slot;
                for(unsigned k = 0; k < g.hs[c] * g.vs[c]; k++) { g.blk_comp[blk++] = c; }
        }
        return t;
}

const char *decode_error_text(unsigned flags)
{
        if(flags & kDecodeBadMarker) { return "a restart marker is missing or out of sequence"; }
        if(flags & kDecodeBadCode) { return "a code that is in no Huffman table"; }
        if(flags & kDecodeBadRun) { return "a run past coefficient 63"; }
        if(flags & kDecodeBadEnd) { return "the scan is truncated, or data is left over behind its last block"; }
        if(flags & kDecodeBadDc) { return "a DC value outside int16"; }
        return "the block count disagrees with the decoder's state";
}

struct DecodeTake {
        size_t total = 0;
        size_t operator()(size_t bytes)
        {
                const size_t at = total;
                total += round_up(bytes ? bytes : 1, 256);
                return at;
        }
};

// rounds queued before the change counters are first read back, and between two reads after that
constexpr unsigned kDecodeFirstGroup = 3, kDecodeGroup = 4;

}  // namespace

// The decoder: p's scan from `data` (the entropy-coded bytes p.info.scan_begin.., HOST memory, or DEVICE memory of `device` read in
// place) into the device grids coef[c] (blocks_w * blocks_h * 64 int16 each), on `stream`, which has been waited for on return.  One
// pooled block holds every intermediate and goes back before returning.  stats may be NULL.
int j2p_decode_file(int device, hipStream_t stream, const j2p_jpeg_parsed *parsed, const uint8_t *data, bool data_on_device, unsigned S,
                    int16_t *const coef[3], j2p_decode_stats *stats)
{
        const j2p_jpeg_parsed &p = *parsed;
        const j2p_jpeg_info &f = p.info;
        if(S == 0) { S = J2P_DECODE_SUBSEQUENCE_BITS; }
        if(S < J2P_DECODE_SUBSEQUENCE_MIN || S > J2P_DECODE_SUBSEQUENCE_MAX) {
                return j2p_fail(J2P_EINVAL, "decode: %u bits in a subsequence (%u..%u)", S, J2P_DECODE_SUBSEQUENCE_MIN, J2P_DECODE_SUBSEQUENCE_MAX);
        }
        const size_t nraw = f.scan_end - f.scan_begin;
        if(nraw == 0) { return j2p_fail(J2P_EFORMAT, "jpeg: the scan holds no data"); }
        const unsigned long long bound = ((unsigned long long)nraw * 8 + S - 1) / S + f.intervals;
        const unsigned long long blocks = (unsigned long long)f.mcus_w * f.mcus_h * f.blocks_per_mcu;
        if(bound > 0x7fffffffull || blocks > 0xffffffffull || nraw / kUnstuffChunk > 0x7fffffffull) {
                return j2p_fail(J2P_EINVAL, "decode: %zu bytes of data are too many for subsequences of %u bits", nraw, S);
        }
        const DecodeTables tables = decode_tables(p, S);
        const unsigned nint = f.intervals, nbound = (unsigned)bound, nblocks = tables.g.nblocks;
        const unsigned nchunks = (unsigned)((nraw + kUnstuffChunk - 1) / kUnstuffChunk);
        const auto tiles = [](unsigned n) { return (n + kScanTile - 1) / kScanTile; };
        const size_t clean_room = round_up(nraw + 16, 4);
        DecodeTake take;
        const size_t raw_at = take(data_on_device ? 0 : nraw), clean_at = take(clean_room);
        const size_t keepc_at = take((size_t)nchunks * 4), markc_at = take((size_t)nchunks * 4), keepo_at = take((size_t)nchunks * 8);
        const size_t marko_at = take((size_t)nchunks * 8), keeps_at = take(((size_t)tiles(nchunks) + 1) * 8), marks_at = take(((size_t)tiles(nchunks) + 1) * 8);
        const size_t rst_at = take((size_t)nint * 8), icount_at = take((size_t)nint * 4), first_at = take((size_t)nint * 8);
        const size_t isums_at = take(((size_t)tiles(nint) + 1) * 8);
        const size_t exit_at[2] = {take((size_t)nbound * 8), take((size_t)nbound * 8)};
        const size_t last_at = take((size_t)nbound * 8), done_at = take((size_t)nbound * 4), before_at = take((size_t)nbound * 8);
        const size_t dsums_at = take(((size_t)tiles(nbound) + 1) * 8);
        const size_t diff_at = take((size_t)nblocks * 4), dc_at = take((size_t)nblocks * 8), dcsums_at = take(((size_t)tiles(nblocks) + 1) * 8);
        const size_t tables_at = take(sizeof(DecodeTables)), flags_at = take(256);     // flags: [0] the error word, [1..] the rounds' change counters
        void *block = nullptr;
        size_t block_bytes = 0;
        HIP_TRY(j2p_pool_take(device, take.total, &block, &block_bytes));
        char *const base = static_cast<char *>(block);
        const auto u32 = [&](size_t at) { return reinterpret_cast<unsigned *>(base + at); };
        const auto u64 = [&](size_t at) { return reinterpret_cast<unsigned long long *>(base + at); };
        unsigned *const flags = u32(flags_at);
        // everything below leaves through `finish`, which gives the block back once the stream is idle
        const auto finish = [&](int rc) {
                (void)hipStreamSynchronize(stream);
                j2p_pool_give(device, block, block_bytes);
                return rc;
        };
        const auto failed = [&](hipError_t e, const char *what) { return finish(j2p_fail(J2P_EDEVICE, "decode: %s: %s", what, hipGetErrorString(e))); };

        const auto t_begin = std::chrono::steady_clock::now();
        const uint8_t *raw = data;
        hipError_t e = hipSuccess;
        if(!data_on_device) {
                e = hipMemcpyAsync(base + raw_at, data, nraw, hipMemcpyHostToDevice, stream);
                raw = reinterpret_cast<const uint8_t *>(base + raw_at);
        }
        if(e == hipSuccess) { e = hipMemcpyAsync(base + tables_at, &tables, sizeof(tables), hipMemcpyHostToDevice, stream); }
        if(e == hipSuccess) { e = hipMemsetAsync(base + clean_at, 0xff, clean_room, stream); }
        if(e == hipSuccess) { e = hipMemsetAsync(base + rst_at, 0, (size_t)nint * 8, stream); }
        if(e == hipSuccess) { e = hipMemsetAsync(base + exit_at[0], 0, (size_t)nbound * 8, stream); }
        if(e == hipSuccess) { e = hipMemsetAsync(base + last_at, 0xff, (size_t)nbound * 8, stream); }
        if(e == hipSuccess) { e = hipMemsetAsync(base + done_at, 0, (size_t)nbound * 4, stream); }
        if(e == hipSuccess) { e = hipMemsetAsync(base + diff_at, 0, (size_t)nblocks * 4, stream); }
        if(e == hipSuccess) { e = hipMemsetAsync(flags, 0, 256, stream); }
        if(e != hipSuccess) { return failed(e, "staging"); }
        // the clean stream and the restart markers' places
        hipLaunchKernelGGL(k_unstuff_count, dim3((nchunks + 3) / 4), dim3(256), 0, stream, raw, nraw, nchunks, u32(keepc_at), u32(markc_at));
        queue_scan(stream, u32(keepc_at), nchunks, u64(keeps_at), u64(keepo_at));
        queue_scan(stream, u32(markc_at), nchunks, u64(marks_at), u64(marko_at));
        hipLaunchKernelGGL(k_unstuff_copy, dim3((nchunks + 3) / 4), dim3(256), 0, stream, raw, nraw, nchunks, static_cast<const unsigned long long *>(u64(keepo_at)),
                           static_cast<const unsigned long long *>(u64(marko_at)), nint, reinterpret_cast<uint8_t *>(base + clean_at), clean_room, u64(rst_at),
                           flags);
        // the subsequences of every interval
        DecodeBuffers b;
        b.tables = reinterpret_cast<const DecodeTables *>(base + tables_at);
        b.words = u32(clean_at);
        b.nwords = clean_room / 4;
        b.clean_bytes = u64(keeps_at) + tiles(nchunks);
        b.nmarkers = u64(marks_at) + tiles(nchunks);
        b.rst = u64(rst_at);
        b.first = u64(first_at);
        b.nsub = u64(isums_at) + tiles(nint);
        b.error = flags;
        hipLaunchKernelGGL(k_decode_intervals, dim3((nint + 255) / 256), dim3(256), 0, stream, b, nint, S, u32(icount_at));
        queue_scan(stream, u32(icount_at), nint, u64(isums_at), u64(first_at));
        // rounds until no entry state changes: at most one per subsequence of the longest interval, and one that finds nothing to do
        j2p_decode_stats st;
        memset(&st, 0, sizeof(st));
        st.intervals = nint;
        unsigned rounds = 0;
        bool settled = false;
        while(!settled) {
                if(rounds > nbound) { return finish(j2p_fail(J2P_EFORMAT, "jpeg: the decoder's states did not settle in %u rounds", rounds)); }
                const unsigned group = rounds == 0 ? kDecodeFirstGroup : kDecodeGroup;
                if(rounds) { (void)hipMemsetAsync(flags + 1, 0, group * 4, stream); }
                for(unsigned q = 0; q < group; q++, rounds++) {
                        hipLaunchKernelGGL(k_decode_sync, dim3((nbound + 255) / 256), dim3(256), 0, stream, b, nbound,
                                           static_cast<const unsigned long long *>(u64(exit_at[rounds & 1])), u64(exit_at[(rounds + 1) & 1]), u64(last_at),
                                           u32(done_at), flags + 1 + q);
                }
                unsigned seen[1 + kDecodeGroup] = {0};
                unsigned long long totals[2] = {0, 0};
                e = hipMemcpyAsync(seen, flags, (1 + group) * 4, hipMemcpyDeviceToHost, stream);
                if(e == hipSuccess) { e = hipMemcpyAsync(&totals[0], b.nsub, 8, hipMemcpyDeviceToHost, stream); }
                if(e == hipSuccess) { e = hipMemcpyAsync(&totals[1], b.clean_bytes, 8, hipMemcpyDeviceToHost, stream); }
                if(e == hipSuccess) { e = hipStreamSynchronize(stream); }
                if(e != hipSuccess) { return failed(e, "rounds"); }
                if(seen[0]) { return finish(j2p_fail(J2P_EFORMAT, "jpeg: %s", decode_error_text(seen[0]))); }
                st.subsequences = (unsigned)totals[0];
                st.data_bytes = totals[1];
                for(unsigned q = 0; q < group && !settled; q++) {
                        if(seen[1 + q] == 0) {
                                settled = true;
                        } else {
                                if(st.rounds < J2P_DECODE_STATS_ROUNDS) { st.recomputed[st.rounds] = seen[1 + q]; }
                                st.rounds++;
                        }
                }
        }
        const unsigned long long *const exits = u64(exit_at[rounds & 1]);       // what the last round queued wrote
        // the block ordinals, the ACs and the DC differences, the DCs
        queue_scan(stream, u32(done_at), nbound, u64(dsums_at), u64(before_at));
        DecodeOut o;
        memset(&o, 0, sizeof(o));
        for(unsigned c = 0; c < f.ncomp; c++) {
                o.coef[c] = coef[c];
                (void)hipMemsetAsync(coef[c], 0, (size_t)f.comp[c].blocks_w * f.comp[c].blocks_h * 64 * sizeof(int16_t), stream);
        }
        o.diff = u32(diff_at);
        hipLaunchKernelGGL(k_decode_write, dim3((nbound + 255) / 256), dim3(256), 0, stream, b, nbound, exits, static_cast<const unsigned long long *>(u64(before_at)), o);
        queue_scan(stream, u32(diff_at), nblocks, u64(dcsums_at), u64(dc_at));
        hipLaunchKernelGGL(k_decode_dc, dim3((nblocks + 255) / 256), dim3(256), 0, stream, b.tables, static_cast<const unsigned *>(u32(diff_at)),
                           static_cast<const unsigned long long *>(u64(dc_at)), o, flags);
        unsigned bad = 0;
        e = hipGetLastError();
        if(e == hipSuccess) { e = hipMemcpyAsync(&bad, flags, 4, hipMemcpyDeviceToHost, stream); }
        if(e == hipSuccess) { e = hipStreamSynchronize(stream); }
        if(e != hipSuccess) { return failed(e, "the final pass"); }
        if(bad) { return finish(j2p_fail(J2P_EFORMAT, "jpeg: %s", decode_error_text(bad))); }
        st.decode_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
        if(stats) { *stats = st; }
        return finish(J2P_OK);
}

// the file on the host for the parse: `file` itself, or a copy of device memory in `copy`; *on_device, *device_of: where it lives
int j2p_decode_fetch(const uint8_t *file, size_t size, uint8_t **copy, bool *on_device, int *device_of)
{
        *copy = nullptr;
        *on_device = false;
        if(!file || size == 0) { return j2p_fail(J2P_EINVAL, "NULL argument"); }
        int where = -1;
        const int kind = j2p_memory_of_pointer(file, &where);
        if(kind == J2P_MEMORY_OTHER) { return j2p_fail(J2P_EINVAL, "jpeg: the file lies in managed or unknown memory (plain device memory, or host memory)"); }
        if(kind == J2P_MEMORY_DEVICE) {
                *copy = static_cast<uint8_t *>(malloc(size));
                if(!*copy) { return j2p_fail(J2P_ENOMEM, "out of memory"); }
                if(const hipError_t e = hipMemcpy(*copy, file, size, hipMemcpyDeviceToHost); e != hipSuccess) {
                        free(*copy);
                        *copy = nullptr;
                        return j2p_fail(J2P_EDEVICE, "jpeg: reading the file: %s", hipGetErrorString(e));
                }
                *on_device = true;
                *device_of = where;
        }
        return J2P_OK;
}

extern "C" {

int j2p_entropy_decode_ex(int device, const uint8_t *file, size_t size, int16_t *const coef_host[3], uint16_t quant[3][64], j2p_jpeg_info *info,
                          unsigned subsequence_bits, j2p_decode_stats *stats)
{
        if(!coef_host) { return j2p_fail(J2P_EINVAL, "NULL argument"); }
        if(subsequence_bits && (subsequence_bits < J2P_DECODE_SUBSEQUENCE_MIN || subsequence_bits > J2P_DECODE_SUBSEQUENCE_MAX)) {
                return j2p_fail(J2P_EINVAL, "decode: %u bits in a subsequence (%u..%u)", subsequence_bits, J2P_DECODE_SUBSEQUENCE_MIN, J2P_DECODE_SUBSEQUENCE_MAX);
        }
        uint8_t *copy = nullptr;
        bool on_device = false;
        int where = -1;
        if(const int rc = j2p_decode_fetch(file, size, &copy, &on_device, &where); rc != J2P_OK) { return rc; }
        j2p_jpeg_parsed *parsed = static_cast<j2p_jpeg_parsed *>(malloc(sizeof(j2p_jpeg_parsed)));
        if(!parsed) {
                free(copy);
                return j2p_fail(J2P_ENOMEM, "out of memory");
        }
        void *block = nullptr;
        size_t block_bytes = 0;
        hipStream_t stream = nullptr;
        const int rc = [&]() -> int {
                if(const int prc = j2p_jpeg_parse_full(copy ? copy : file, size, parsed); prc != J2P_OK) { return prc; }
                const j2p_jpeg_info &f = parsed->info;
                for(unsigned c = 0; c < f.ncomp; c++) {
                        if(!coef_host[c]) { return j2p_fail(J2P_EINVAL, "decode: component %u has no room for its coefficients", c); }
                }
                int have = 0;
                if(hipGetDeviceCount(&have) != hipSuccess || have <= 0) { return j2p_fail(J2P_EDEVICE, "no HIP device available"); }
                if(device < 0 || device >= have) { return j2p_fail(J2P_EINVAL, "device %d out of range (0..%d)", device, have - 1); }
                if(on_device && where != device) { return j2p_fail(J2P_EINVAL, "jpeg: the file lies on device %d, the decode runs on %d", where, device); }
                DeviceGuard guard(device);
                HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
                size_t at[3] = {0, 0, 0}, bytes = 0;
                for(unsigned c = 0; c < f.ncomp; c++) {
                        at[c] = bytes;
                        bytes += round_up((size_t)f.comp[c].blocks_w * f.comp[c].blocks_h * 64 * sizeof(int16_t), 256);
                }
                HIP_TRY(j2p_pool_take(device, bytes, &block, &block_bytes));
                int16_t *coef[3] = {nullptr, nullptr, nullptr};
                for(unsigned c = 0; c < f.ncomp; c++) { coef[c] = reinterpret_cast<int16_t *>(static_cast<char *>(block) + at[c]); }
                if(const int drc = j2p_decode_file(device, stream, parsed, file + f.scan_begin, on_device, subsequence_bits, coef, stats); drc != J2P_OK) {
                        return drc;
                }
                // one staging copy down, so that nothing reaches the caller's arrays unless all of it does
                int16_t *staged = static_cast<int16_t *>(malloc(bytes ? bytes : 1));
                if(!staged) { return j2p_fail(J2P_ENOMEM, "out of memory"); }
                if(const hipError_t e = hipMemcpy(staged, block, bytes, hipMemcpyDeviceToHost); e != hipSuccess) {
                        free(staged);
                        return j2p_fail(J2P_EDEVICE, "decode: %s", hipGetErrorString(e));
                }
                for(unsigned c = 0; c < f.ncomp; c++) {
                        memcpy(coef_host[c], reinterpret_cast<char *>(staged) + at[c], (size_t)f.comp[c].blocks_w * f.comp[c].blocks_h * 64 * sizeof(int16_t));
                        if(quant) { memcpy(quant[c], f.comp[c].quant, sizeof(f.comp[c].quant)); }
                }
                free(staged);
                if(info) { *info = f; }
                return J2P_OK;
        }();
        if(stream) {
                (void)hipStreamSynchronize(stream);
                (void)hipStreamDestroy(stream);
        }
        if(block) { j2p_pool_give(device, block, block_bytes); }
        free(parsed);
        free(copy);
        return rc;
}

int j2p_entropy_decode(int device, const uint8_t *file, size_t size, int16_t *const coef_host[3], uint16_t quant[3][64], j2p_jpeg_info *info)
{
        return j2p_entropy_decode_ex(device, file, size, coef_host, quant, info, 0, nullptr);
}

}  // extern "C"
