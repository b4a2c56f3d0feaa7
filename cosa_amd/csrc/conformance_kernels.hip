// conformance_kernels.hip -- the pre-registered CAM criterion (rules (a) and (b)) per plane on the device (section 20).
//
// One workgroup per (image, class) plane reduces six maxima and one count over the plane in a fixed tree (per-thread strided scan, wavefront
// butterfly, four partials through LDS in index order) and thread 0 forms the figures and the verdict in float64.  Maxima and integer counts
// are exact whatever the order, and the order is fixed anyway: the same bytes on every run.  NaN never enters a maximum (fmax drops it); a
// plane of the mode under test that holds a non-finite element fails.
#include "wave_reduce.hpp"
#include <cmath>

namespace cosa {
namespace {

__global__ __launch_bounds__(256) void conformance_planes_kernel(const float *__restrict__ camA, const float *__restrict__ cam32,
                                                                 const double *__restrict__ cam64, const float *__restrict__ active,
                                                                 const double *__restrict__ peak64, const double *__restrict__ rawmax64, int HW,
                                                                 double cam_bar, double cond_max, double fp64_factor, double *__restrict__ fig,
                                                                 int *__restrict__ verdict)
{
    __shared__ double sh[4][4];
    __shared__ unsigned shn[4];
    const int plane = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    double *f = fig + (size_t)plane * COSA_CONFORMANCE_FIGS;
    int *vd = verdict + (size_t)plane * 2;
    if (active && active[plane] == 0.0f) {          // ignored: a row of zeros, verdict -1
        if (tid < COSA_CONFORMANCE_FIGS) f[tid] = 0.0;
        if (tid == 0) { vd[0] = -1; vd[1] = 0; }
        return;
    }
    const float *a = camA + (size_t)plane * HW, *c32 = cam32 + (size_t)plane * HW;
    const double *c64 = cam64 + (size_t)plane * HW;
    double d = 0.0, m32 = 0.0, e_ref = 0.0, e_hip = 0.0;
    unsigned bad = 0;
    for (int i = tid; i < HW; i += 256) {
        const double av = (double)a[i], cv = (double)c32[i], rv = c64[i];
        bad += nonfinite_bits(a[i]);
        d = fmax(d, fabs(av - cv));
        m32 = fmax(m32, fabs(cv));
        e_ref = fmax(e_ref, fabs(cv - rv));
        e_hip = fmax(e_hip, fabs(av - rv));
    }
    d = wave_max(d); m32 = wave_max(m32); e_ref = wave_max(e_ref); e_hip = wave_max(e_hip);
    bad = wave_sum32(bad);
    if (lane == 0) { sh[wid][0] = d; sh[wid][1] = m32; sh[wid][2] = e_ref; sh[wid][3] = e_hip; shn[wid] = bad; }
    __syncthreads();
    if (tid != 0) return;
    for (int i = 1; i < 4; i++) {
        d = fmax(d, sh[i][0]); m32 = fmax(m32, sh[i][1]); e_ref = fmax(e_ref, sh[i][2]); e_hip = fmax(e_hip, sh[i][3]);
        bad += shn[i];
    }
    const double peak = peak64[plane], rawmax = rawmax64[plane];
    const double lit = d / fmax(m32, 1e-6);
    const double cond = rawmax / peak;
    const double own = d * peak / fmax(rawmax, 1e-30);
    const double bound = cam_bar + fp64_factor * e_ref;
    int v;
    if (bad) v = 2;
    else if (lit <= cam_bar) v = 0;
    else if (cond > cond_max && own <= cam_bar && e_hip <= bound) v = 1;
    else v = 2;
    f[0] = d; f[1] = lit; f[2] = cond; f[3] = own; f[4] = e_ref; f[5] = e_hip; f[6] = bound; f[7] = m32;
    vd[0] = v;
    vd[1] = (int)bad;
}

}  // namespace
}  // namespace cosa

using namespace cosa;

extern "C" int cosa_conformance_planes(const float *camA, const float *cam32, const double *cam64, const float *active, const double *peak64,
                                       const double *rawmax64, int planes, int HW, double cam_bar, double cond_max, double fp64_factor, double *fig,
                                       int *verdict, void *stream)
{
    COSA_REQUIRE(camA && cam32 && cam64 && peak64 && rawmax64 && fig && verdict, "cosa_conformance_planes: null operand");
    COSA_REQUIRE(planes >= 1 && HW >= 1, "cosa_conformance_planes: planes >= 1, HW >= 1 (got %d, %d)", planes, HW);
    hipLaunchKernelGGL(conformance_planes_kernel, dim3((unsigned)planes), dim3(256), 0, as_stream(stream), camA, cam32, cam64, active, peak64,
                       rawmax64, HW, cam_bar, cond_max, fp64_factor, fig, verdict);
    COSA_LAUNCH_CHECK();
    return COSA_OK;
}
