// weight_planes.hip - pre-split weight images (QA_GEMM_PRESPLIT; layout and split in split_planes.h): image builder and registry.
// The weights of a model never change after load, yet the K loop splits a weight tile again for every row tile of every launch.
// A WeightStore therefore builds the plane image of its whole blob once, at load, and attaches it here; launch_conv_gemm looks the
// launch's weight pointer up and, when an image covers it, takes the kernel instance whose B staging copies 16-byte plane units
// instead of splitting.  The lookup is by address, so row slices and hand-built views of a stored weight find their planes too.
#include <algorithm>
#include <mutex>
#include <vector>

#include "common.h"
#include "split_planes.h"

namespace qa {

__global__ __launch_bounds__(256) void weight_planes_kernel(const float* __restrict__ w, long long groups, char* __restrict__ planes) {
    for (long long g = blockIdx.x * 256LL + threadIdx.x; g < groups; g += gridDim.x * 256LL) {
        u32x2 h0, m0, l0, h1, m1, l1;
        split4_rne(*reinterpret_cast<const f32x4*>(w + g * 8), h0, m0, l0);
        split4_rne(*reinterpret_cast<const f32x4*>(w + g * 8 + 4), h1, m1, l1);
        u32x4* out = reinterpret_cast<u32x4*>(planes + g * PLANE_GROUP_BYTES);
        out[0] = u32x4{h0[0], h0[1], h1[0], h1[1]};
        out[1] = u32x4{m0[0], m0[1], m1[0], m1[1]};
        out[2] = u32x4{l0[0], l0[1], l1[0], l1[1]};
    }
}

int launch_weight_planes(const float* w, long long n, void* planes, hipStream_t stream) {
    QA_REQUIRE(w && planes && n >= 0 && n % 8 == 0, "weight_planes: null pointer or n=%lld not a multiple of 8", n);
    QA_REQUIRE(((uintptr_t)w % 16) == 0 && ((uintptr_t)planes % 16) == 0, "weight_planes: w / planes must be 16-byte aligned");
    if (n == 0) return QA_OK;
    const long long groups = n / 8;
    const unsigned grid = (unsigned)std::min<long long>(ceil_div(groups, 256), 256 * 64);
    hipLaunchKernelGGL(weight_planes_kernel, dim3(grid), dim3(256), 0, stream, w, groups, static_cast<char*>(planes));
    QA_LAUNCH_CHECK();
    return QA_OK;
}

namespace {
struct PlaneImage {
    const float* w;
    long long n;
    const char* planes;
};
std::mutex g_planes_mu;
std::vector<PlaneImage> g_planes;  // a handful of entries: one per loaded weight store
}  // namespace

int weight_planes_attach(const float* w, long long n, const void* planes) {
    QA_REQUIRE(w && planes && n > 0 && n % 8 == 0, "weight_planes_attach: null pointer or n=%lld not a positive multiple of 8", n);
    QA_REQUIRE(((uintptr_t)w % 32) == 0 && ((uintptr_t)planes % 16) == 0, "weight_planes_attach: w must be 32-byte, planes 16-byte aligned");
    std::lock_guard<std::mutex> lock(g_planes_mu);
    for (const PlaneImage& im : g_planes)
        QA_REQUIRE(w + n <= im.w || im.w + im.n <= w, "weight_planes_attach: the range overlaps an attached image");
    g_planes.push_back(PlaneImage{w, n, static_cast<const char*>(planes)});
    return QA_OK;
}

void weight_planes_detach(const float* w) {
    std::lock_guard<std::mutex> lock(g_planes_mu);
    for (size_t i = 0; i < g_planes.size(); ++i)
        if (g_planes[i].w == w) {
            g_planes.erase(g_planes.begin() + (long)i);
            return;
        }
}

long long weight_planes_bytes() {
    std::lock_guard<std::mutex> lock(g_planes_mu);
    long long total = 0;
    for (const PlaneImage& im : g_planes) total += im.n / 8 * PLANE_GROUP_BYTES;
    return total;
}

// the planes of w[0 .. n) when one attached image covers them and w sits on an 8-float group of it; else nullptr (split in the loop)
const char* weight_planes_find(const float* w, long long n) {
    std::lock_guard<std::mutex> lock(g_planes_mu);
    for (const PlaneImage& im : g_planes)
        if (w >= im.w && w + n <= im.w + im.n && ((w - im.w) & 7) == 0) return im.planes + plane_byte_offset(w - im.w, 0);
    return nullptr;
}

}  // namespace qa
