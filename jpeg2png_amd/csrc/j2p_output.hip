// jpeg2png_amd — the output stage: solved planes to samples on the host (PNG), to a strided tensor in device memory, whole
// or cropped and resized (area, or triangle / cubic taps; several such outputs in one call), to quantised JPEG
// coefficients, and — those handed to the codec's coder (j2p_codec.hip) — to the entropy-coded JPEG file itself; and samples
// left in device memory for the codec's PNG coder, to the PNG file (include/jpeg2png_amd.h: the j2p_planes_* functions).
// Every form of an oriented solver (j2p_solver_set_orientation) runs on the solver's upright planes instead: "upright planes" below.
//
// A translation unit of its own, with its own device code (j2p_output_kernels.hip.h): it changes more often than the solver
// and must not recompile the solver's kernels.  It sees of a solver what j2p_solver_view and j2p_solver_row give
// (j2p_internal.h), never the solver's struct, its halo or its arena; j2p_solver_scratch lends it memory that lives with the
// solver.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "jpeg2png_amd.h"
#include "j2p_internal.h"
#include "j2p_hip_host.h"
#include "j2p_output_kernels.hip.h"

using namespace j2p;

extern "C" {

// ---- upright planes: k_upright_rows, k_upright_transpose ----
// An oriented solver (j2p_solver_set_orientation, 2..8) shows the forms below not its canvas but UPRIGHT planes: the
// permutation of the current iterate, replication included (include/jpeg2png_amd.h, "Upright output").  This is the one place
// that knows: form_view gives the canvas a call's extents are checked against, plane_rows the address of a row — and notes in
// the call's Upright which planes have to be permuted — and upright_queue, which a form calls once, after its last check and
// before its first launch, queues those permutations.  An unoriented solver passes through all three untouched: no launch, no
// allocation.
// Ordering rule: every upright plane of a call — also those of OTHER solvers (`-s`: three solvers, one channel each) — lies in the
// block of the call's first solver, the owner, on whose stream the form launches, and is written there: the block is written,
// read and regrown in that one stream's order only, so no call can overwrite or give back what another stream still reads.  The
// other solvers' iterates are read after their streams have been waited for, as the forms always did.
struct Upright {
        j2p_solver *owner = nullptr;    // the first oriented plane's solver: planes[0].solver of the call
        unsigned slots = 3;             // planes the call reads at most (set by the caller before plane_rows)
        unsigned n = 0;                 // distinct planes noted
        struct Plane {
                const j2p_solver *solver;
                unsigned channel;
                const float *src;       // row 0 of the solver's iterate
                unsigned src_stride;    // that solver's canvas width: solvers of one call may differ in it
                float *dst;
        } plane[3];
        UprightGeom g;                  // the same for all of them (same_orientation) but for src_stride
        bool transposed = false;        // orientations 5..8
};

static j2p_solver_view form_view(const j2p_solver *solver)
{
        j2p_solver_view v = j2p_solver_view_of(solver);
        if(v.orientation > 1) {
                const bool transposed = v.orientation >= 5;
                v.W = ((transposed ? v.orient_h : v.orient_w) + 15) / 16 * 16;
                v.H = ((transposed ? v.orient_w : v.orient_h) + 15) / 16 * 16;
                v.row0 = 0;             // (whole: band solvers take no orientation)
                v.rows = v.H;
        }
        return v;
}

// true when b's planes can stand next to a's in one call: the same orientation of the same source image
static bool same_orientation(const j2p_solver_view &a, const j2p_solver_view &b)
{
        const bool oa = a.orientation > 1, ob = b.orientation > 1;
        return oa == ob && (!oa || (a.orientation == b.orientation && a.orient_w == b.orient_w && a.orient_h == b.orient_h));
}

// the address of row y of (solver, channel) as a form sees it, s = form_view(solver): the rows after it follow at s.W floats
static int plane_rows(const j2p_plane_ref &plane, const j2p_solver_view &s, unsigned y, Upright &up, const float **row)
{
        if(s.orientation <= 1) { return j2p_solver_row(plane.solver, plane.channel, y, row); }
        if(plane.channel >= s.nch || y >= s.H) { return j2p_fail(J2P_EINVAL, "row %u of channel %u is not one of the upright canvas", y, plane.channel); }
        for(unsigned k = 0; k < up.n; k++) {
                if(up.plane[k].solver == plane.solver && up.plane[k].channel == plane.channel) {       // the same plane twice in one call: permuted once
                        *row = up.plane[k].dst + (size_t)y * s.W;
                        return J2P_OK;
                }
        }
        if(up.n == 3) { return j2p_fail(J2P_EINVAL, "more than three planes in one call"); }
        if(!up.owner) { up.owner = plane.solver; }
        const size_t plane_floats = (size_t)s.W * s.H;
        // (the same size for every plane of a call — at least the owner's channels, so that a joint solver's block has one size
        // whatever a call reads: only a call's first request can move the block)
        const unsigned owner_nch = j2p_solver_view_of(up.owner).nch, slots = up.slots > owner_nch ? up.slots : owner_nch;
        float *base = nullptr;
        if(const int rc = j2p_solver_upright(up.owner, plane_floats * slots * sizeof(float), &base); rc != J2P_OK) { return rc; }
        Upright::Plane &P = up.plane[up.n];
        P.solver = plane.solver;
        P.channel = plane.channel;
        P.dst = base + plane_floats * up.n;
        if(const int rc = j2p_solver_row(plane.solver, plane.channel, 0, &P.src); rc != J2P_OK) { return rc; }
        P.src_stride = j2p_solver_view_of(plane.solver).W;
        up.n++;
        *row = P.dst + (size_t)y * s.W;
        const bool transposed = s.orientation >= 5;
        up.transposed = transposed;
        UprightGeom &g = up.g;
        g.w = s.orient_w;
        g.h = s.orient_h;
        g.uw = transposed ? s.orient_h : s.orient_w;
        g.uh = transposed ? s.orient_w : s.orient_h;
        g.UW = s.W;
        g.UH = s.H;
        g.src_stride = 0;               // (per launch: upright_queue)
        g.flip_x = s.orientation == 2 || s.orientation == 3 || s.orientation == 7 || s.orientation == 8;
        g.flip_y = s.orientation == 3 || s.orientation == 4 || s.orientation == 6 || s.orientation == 7;
        return J2P_OK;
}

// Queues what plane_rows noted on `stream`, the owner's, on which the form launches: one launch for the planes that share a
// source stride (all of a joint solver's), so at most one per solver.  The caller has waited for the other solvers' streams.
static int upright_queue(const Upright &up, hipStream_t stream)
{
        bool done[3] = {false, false, false};
        for(unsigned i = 0; i < up.n; i++) {
                if(done[i]) { continue; }
                UprightGeom g = up.g;
                g.src_stride = up.plane[i].src_stride;
                const float *src[3] = {nullptr, nullptr, nullptr};
                float *dst[3] = {nullptr, nullptr, nullptr};
                unsigned n = 0;
                for(unsigned k = i; k < up.n; k++) {
                        if(done[k] || up.plane[k].src_stride != g.src_stride) { continue; }
                        src[n] = up.plane[k].src;
                        dst[n] = up.plane[k].dst;
                        done[k] = true;
                        n++;
                }
                const UprightPlanes p = {src[0], src[1], src[2], dst[0], dst[1], dst[2]};
                if(up.transposed) {
                        hipLaunchKernelGGL(k_upright_transpose, dim3((g.UW + kUprightTile - 1) / kUprightTile, (g.UH + kUprightTile - 1) / kUprightTile, n),
                                           dim3(256), 0, stream, p, g);
                } else {
                        hipLaunchKernelGGL(k_upright_rows, dim3((g.UW + 255) / 256, (g.UH + 3) / 4, n), dim3(256), 0, stream, p, g);
                }
                const hipError_t e = hipGetLastError();
                if(e != hipSuccess) { return j2p_fail(J2P_EDEVICE, "upright planes: %s", hipGetErrorString(e)); }
        }
        return J2P_OK;
}

// What the conversions of solved planes start from: rows [y0, y1) x w columns of the image from nplane (3 or 1) (solver,
// channel) pairs on one device that all hold those canvas rows.  Checks arguments and state, gives per plane the first of
// those rows in the current iterate and its stride in floats and the view of planes[0].solver, and waits for the streams of
// the other solvers: the caller launches on planes[0].solver's.  `whole`: called as a whole-canvas form, which band solvers
// refuse.  what: "to_rgb", "to_grey" or "to_tensor", for the messages.  Oriented solvers: canvas, rows and view are those of the
// upright planes (form_view), and `up` is what the caller hands to upright_queue before it launches.
static int resolve_rows(const char *what, const j2p_plane_ref *planes, unsigned nplane, bool whole, unsigned w, unsigned y0, unsigned y1,
                        const float *ptr[3], unsigned stride[3], j2p_solver_view &first, Upright &up)
{
        if(w == 0 || y0 >= y1) { return j2p_fail(J2P_EINVAL, whole ? "empty image" : "empty row range"); }
        for(unsigned i = 0; whole && i < nplane; i++) {
                if(planes[i].solver && !j2p_solver_view_of(planes[i].solver).whole) {
                        return j2p_fail(J2P_ESTATE, "%s needs whole-canvas solvers (bands: j2p_planes_rows_%s)", what, what);
                }
        }
        for(unsigned i = 0; i < 3; i++) { ptr[i] = nullptr; stride[i] = 0; }
        up.slots = nplane;
        for(unsigned i = 0; i < nplane; i++) {
                const j2p_solver_view s = planes[i].solver ? form_view(planes[i].solver) : j2p_solver_view{};
                if(!planes[i].solver || planes[i].channel >= s.nch) { return j2p_fail(J2P_EINVAL, "plane %u: bad solver/channel", i); }
                if(i == 0) { first = s; }
                if(s.device != first.device) { return j2p_fail(J2P_EINVAL, "planes live on different devices"); }
                if(!whole && s.orientation > 1) { return j2p_fail(J2P_ESTATE, "the rows forms take no oriented solver (plane %u)", i); }
                if(!same_orientation(first, s)) { return j2p_fail(J2P_EINVAL, "plane %u: another orientation or source size than plane 0's", i); }
                if(s.W < w || y0 < s.row0 || y1 > s.row0 + s.rows) {
                        return j2p_fail(J2P_EINVAL, "plane %u: rows [%u,%u) x %u columns are not inside the solver's [%u,%u) x %u", i, y0, y1, w,
                                    s.row0, s.row0 + s.rows, s.W);
                }
                if(s.mid_iteration) { return j2p_fail(J2P_ESTATE, "%s between the two phases of an iteration", what); }
                if(const int rc = plane_rows(planes[i], s, y0, up, &ptr[i]); rc != J2P_OK) { return rc; }
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
        Upright up;
        if(const int rc = resolve_rows(what, planes, nplane, whole, w, y0, y1, ptr, stride, s0, up); rc != J2P_OK) { return rc; }
        const unsigned h = y1 - y0;
        DeviceGuard guard(s0.device);
        const size_t bytes = (size_t)w * h * (size_t)nplane * (bits / 8);
        void *dout = nullptr;
        size_t dout_bytes = 0;
        HIP_TRY(j2p_pool_take(s0.device, bytes, &dout, &dout_bytes));       // pooled like the solvers' arenas: no hipFree per image
        if(const int rc = upright_queue(up, s0.stream); rc != J2P_OK) {
                j2p_pool_give(s0.device, dout, dout_bytes);
                return rc;
        }
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
// planes' first rows and strides, the kernels' view of the destination and the view of planes[0].solver.  In two parts: a call
// of several outputs resolves its planes once (tensor_resolve for its first output) and checks every further destination with
// tensor_destination alone.
static int tensor_destination(const j2p_tensor *out, unsigned nplane, const j2p_solver_view &s0, TensorOut &o);
static int tensor_resolve(const j2p_plane_ref *planes, unsigned nplane, bool whole, unsigned w, unsigned y0, unsigned y1, const j2p_tensor *out,
                          const float *ptr[3], unsigned stride[3], TensorOut &o, j2p_solver_view &s0, Upright &up)
{
        if(!planes || !out) { return j2p_fail(J2P_EINVAL, "NULL argument"); }
        if(nplane != 1 && nplane != 3) { return j2p_fail(J2P_EINVAL, "to_tensor: three planes (RGB) or one (greyscale), not %u", nplane); }
        if(const int rc = resolve_rows("to_tensor", planes, nplane, whole, w, y0, y1, ptr, stride, s0, up); rc != J2P_OK) { return rc; }
        for(unsigned i = 0; i < nplane; i++) {
                // what k_to_tensor's 16-byte loads rest on (see there): true of every solver j2p_solver_create makes
                if(stride[i] % 4 != 0 || reinterpret_cast<uintptr_t>(ptr[i]) % 16 != 0) { return j2p_fail(J2P_ESTATE, "plane %u: canvas rows are not 16-byte aligned", i); }
        }
        return tensor_destination(out, nplane, s0, o);
}
static int tensor_destination(const j2p_tensor *out, unsigned nplane, const j2p_solver_view &s0, TensorOut &o)
{
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
        Upright up;
        if(const int rc = tensor_resolve(planes, nplane, whole, w, y0, y1, out, ptr, stride, o, s0, up); rc != J2P_OK) { return rc; }
        DeviceGuard guard(s0.device);
        if(const int rc = upright_queue(up, s0.stream); rc != J2P_OK) { return rc; }
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
        Upright up;
        if(const int rc = tensor_resolve(planes, nplane, true, w, 0, h, out, ptr, stride, o, s0, up); rc != J2P_OK) { return rc; }
        DeviceGuard guard(s0.device);
        if(const int rc = upright_queue(up, s0.stream); rc != J2P_OK) { return rc; }
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
        Upright up;
        if(const int rc = tensor_resolve(planes, nplane, true, w, 0, h, out, ptr, stride, o, s0, up); rc != J2P_OK) { return rc; }
        DeviceGuard guard(s0.device);
        const OutputPlan p = plan_output(*r);
        void *scratch = nullptr;
        if(const int rc = j2p_solver_scratch(planes[0].solver, p.words * 4, &scratch); rc != J2P_OK) { return rc; }
        if(const int rc = upright_queue(up, s0.stream); rc != J2P_OK) { return rc; }
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
        Upright up;
        for(unsigned i = 0; i < n; i++) {
                const int rc = i == 0 ? tensor_resolve(planes, nplane, true, w, 0, h, &outs[0].t, ptr, stride, o[0], s0, up)
                                      : tensor_destination(&outs[i].t, nplane, s0, o[i]);
                if(rc != J2P_OK) { return rc; }
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
        if(const int rc = upright_queue(up, s0.stream); rc != J2P_OK) { return rc; }
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
                          unsigned r1, const uint16_t quant_table[64], QuantiseLaunch &q, Upright &up)
{
        if(!plane || !quant_table) { return j2p_fail(J2P_EINVAL, "NULL argument"); }
        if(blocks_w == 0 || r0 >= r1) { return j2p_fail(J2P_EINVAL, whole ? "empty image" : "empty row range"); }
        const j2p_solver_view s = plane->solver ? form_view(plane->solver) : j2p_solver_view{};
        if(whole && plane->solver && !s.whole) {
                return j2p_fail(J2P_ESTATE, "to_coefficients needs a whole-canvas solver (bands: the j2p_planes_rows_to_coefficients forms)");
        }
        if(sub_w < 1 || sub_w > 2 || sub_h < 1 || sub_h > 2) {
                return j2p_fail(J2P_EINVAL, "to_coefficients: sampling factors %ux%u (1 and 2 are supported)", sub_w, sub_h);
        }
        if(!plane->solver || plane->channel >= s.nch) { return j2p_fail(J2P_EINVAL, "plane 0: bad solver/channel"); }
        if(!whole && s.orientation > 1) { return j2p_fail(J2P_ESTATE, "the rows forms take no oriented solver"); }
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
        if(const int rc = plane_rows(*plane, s, first, up, &src); rc != J2P_OK) { return rc; }
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
        Upright up;
        up.slots = 1;
        if(const int rc = quantise_check(plane, whole, sub_w, sub_h, blocks_w, r0, r1, quant_table, q, up); rc != J2P_OK) { return rc; }
        const j2p_solver_view &s = q.s;
        DeviceGuard guard(s.device);
        const size_t bytes = (size_t)blocks_w * (r1 - r0) * 64 * sizeof(int16_t);
        void *dout = nullptr;
        size_t dout_bytes = 0;
        HIP_TRY(j2p_pool_take(s.device, bytes, &dout, &dout_bytes));
        if(const int rc = upright_queue(up, s.stream); rc != J2P_OK) {
                j2p_pool_give(s.device, dout, dout_bytes);
                return rc;
        }
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

// a file coder's `memory` (j2p_internal.h) that is owner's scratch: another block, its contents lost, once a request is beyond it
static std::function<int(size_t, void **, bool *)> scratch_memory(j2p_solver *owner)
{
        return [owner](size_t bytes, void **p, bool *moved) {
                *moved = j2p_solver_scratch_bytes(owner) < bytes;
                return j2p_solver_scratch(owner, bytes, p);
        };
}

// the JPEG file: the planes quantised into the coder's block (j2p_codec.hip: j2p_encode_options, which chooses the coder by the
// record and hands the restart intervals on), which is the first solver's scratch
static int planes_to_jpeg(const j2p_plane_ref planes[], unsigned nplane, const j2p_jpeg *spec, uint8_t *out_host, size_t capacity, size_t *size,
                          const j2p_jpeg_options *options)
{
        if(!planes || !size) { return j2p_fail(J2P_EINVAL, "NULL argument"); }
        if(const char *why = j2p_jpeg_options_error(options)) { return j2p_fail(J2P_EINVAL, "%s", why); }
        if(const char *why = j2p_jpeg_error(spec, nplane)) { return j2p_fail(J2P_EINVAL, "%s", why); }
        const j2p_scan_grids g = j2p_scan_grids_of(*spec, nplane);
        // every check of every plane, before anything is queued
        QuantiseLaunch q[3];
        Upright up;
        up.slots = nplane;
        for(unsigned c = 0; c < nplane; c++) {
                const unsigned sx = c ? g.sub_w : 1, sy = c ? g.sub_h : 1;
                if(const int rc = quantise_check(&planes[c], true, sx, sy, g.bw[c], 0, g.bh[c], spec->quant[c], q[c], up); rc != J2P_OK) { return rc; }
                if(q[c].s.device != q[0].s.device) { return j2p_fail(J2P_EINVAL, "planes live on different devices"); }
                if(!same_orientation(q[0].s, q[c].s)) { return j2p_fail(J2P_EINVAL, "plane %u: another orientation or source size than plane 0's", c); }
        }
        DeviceGuard guard(q[0].s.device);
        const hipStream_t stream = q[0].s.stream;
        // everything is queued on planes[0].solver's stream: the other solvers' planes must be complete
        for(unsigned c = 1; c < nplane; c++) {
                if(planes[c].solver != planes[0].solver) { HIP_TRY(hipStreamSynchronize(q[c].s.stream)); }
        }
        if(const int rc = upright_queue(up, stream); rc != J2P_OK) { return rc; }
        const auto memory = scratch_memory(planes[0].solver);
        const auto fill = [&](hipStream_t st, int16_t *const coef[3]) {
                for(unsigned c = 0; c < nplane; c++) { quantise_queue(q[c], c ? g.sub_w : 1, c ? g.sub_h : 1, g.bw[c], 0, g.bh[c], st, coef[c]); }
        };
        return j2p_encode_options(stream, *spec, nplane, *options, memory, fill, out_host, capacity, size);
}

int j2p_planes_to_jpeg_opt(const j2p_plane_ref planes[], unsigned nplane, const j2p_jpeg *spec, uint8_t *out_host, size_t capacity, size_t *size,
                           const j2p_jpeg_options *options)
{
        return planes_to_jpeg(planes, nplane, spec, out_host, capacity, size, options);
}

int j2p_planes_to_jpeg_ex(const j2p_plane_ref planes[], unsigned nplane, const j2p_jpeg *spec, uint8_t *out_host, size_t capacity, size_t *size,
                          unsigned flags)
{
        const j2p_jpeg_options options = {flags, 0, 0, 0};
        return planes_to_jpeg(planes, nplane, spec, out_host, capacity, size, &options);
}

int j2p_planes_to_jpeg_progressive(const j2p_plane_ref planes[], unsigned nplane, const j2p_jpeg *spec, uint8_t *out_host, size_t capacity, size_t *size)
{
        const j2p_jpeg_options options = {0, 1, 0, 0};
        return planes_to_jpeg(planes, nplane, spec, out_host, capacity, size, &options);
}

int j2p_planes_to_jpeg(const j2p_plane_ref planes[], unsigned nplane, const j2p_jpeg *spec, uint8_t *out_host, size_t capacity, size_t *size)
{
        return j2p_planes_to_jpeg_ex(planes, nplane, spec, out_host, capacity, size, 0);
}

// the PNG file: the samples k_to_samples makes for j2p_planes_to_rgb / _grey, left in the coder's block (j2p_codec.hip: j2p_png_write),
// which is the first solver's scratch
int j2p_planes_to_png(const j2p_plane_ref planes[], unsigned nplane, const j2p_png *spec, uint8_t *out_host, size_t capacity, size_t *size)
{
        if(!planes || !size) { return j2p_fail(J2P_EINVAL, "NULL argument"); }
        if(const char *why = j2p_png_error(spec, nplane)) { return j2p_fail(J2P_EINVAL, "%s", why); }
        const float *ptr[3];
        unsigned stride[3];
        j2p_solver_view s0;
        Upright up;
        if(const int rc = resolve_rows(nplane == 3 ? "to_rgb" : "to_grey", planes, nplane, true, spec->width, 0, spec->height, ptr, stride, s0, up);
           rc != J2P_OK) {
                return rc;
        }
        DeviceGuard guard(s0.device);
        if(const int rc = upright_queue(up, s0.stream); rc != J2P_OK) { return rc; }
        const unsigned w = spec->width, h = spec->height, bits = spec->bits;
        return j2p_png_write(
                s0.stream, *spec, nplane, scratch_memory(planes[0].solver),
                [&](hipStream_t st, uint8_t *samples) {
                        hipLaunchKernelGGL(nplane == 3 ? k_to_samples<3> : k_to_samples<1>, dim3(2048), dim3(256), 0, st, ptr[0], stride[0], ptr[1], stride[1],
                                           ptr[2], stride[2], w, h, bits, samples);
                },
                out_host, capacity, size);
}

}  // extern "C"
