// frames.hip -- decoded RGB-D frames to the tensors PCR-CG's loader hands on (ref:datasets/indoor.py:63-78: PIL's
// Resize(size, Image.NEAREST) followed by torchvision's ToTensor, and the `/ 1000.0` of the depth frames), for all the
// frames of a batch of pairs in ONE launch.
//
// Nearest rule (PIL's, not torch.nn.functional.interpolate's): output index i of an axis n_in -> n_out reads input index
// floor((i + 0.5) * n_in / n_out), evaluated in float64 and clamped to n_in - 1.
// Colour: uint8 [F, H, W, 3] -> float32 [F, 3, oh, ow], value = float(v) / 255.0f (an IEEE division, as ToTensor's).
// Depth : uint16 [G, Hd, Wd] -> float32 [G, ohd, owd], value = float(int16(v)) / 1000.0f.  The int16 is the reference's:
// ToTensor reads a 16-bit PNG (PIL mode I;16) through np.int16, so 65535 ("no reading") becomes -0.001 m and every raw
// value of 32768 or more comes out negative.
// One thread per output pixel (a colour thread writes its three channel planes); plain stores, no atomics, no workspace.
#include "common.h"

namespace pcrcg {
namespace {

struct FramesArgs {
    const unsigned char* color; float* color_out;
    const unsigned short* depth; float* depth_out;
    int F, H, W, oh, ow;
    int G, Hd, Wd, ohd, owd;
};

__device__ __forceinline__ int nearest_src(int i, int n_in, int n_out) {
    const int s = (int)floor(((double)i + 0.5) * (double)n_in / (double)n_out);
    return s < n_in - 1 ? s : n_in - 1;
}

// blockIdx.y: the frame (colour frames first, then depth frames); blockIdx.x * 256 + threadIdx.x: its output pixel
__global__ void __launch_bounds__(256) k_prepare_frames(FramesArgs a) {
    const int f = blockIdx.y;
    const long px = (long)blockIdx.x * 256 + threadIdx.x;
    if (f < a.F) {
        if (px >= (long)a.oh * a.ow) return;
        const int y = (int)(px / a.ow), x = (int)(px - (long)y * a.ow);
        const int sy = nearest_src(y, a.H, a.oh), sx = nearest_src(x, a.W, a.ow);
        const unsigned char* p = a.color + (((size_t)f * a.H + sy) * a.W + sx) * 3;
        const size_t plane = (size_t)a.oh * a.ow;
        float* o = a.color_out + (size_t)f * 3 * plane + (size_t)px;
        o[0] = (float)p[0] / 255.0f;
        o[plane] = (float)p[1] / 255.0f;
        o[2 * plane] = (float)p[2] / 255.0f;
    } else {
        const int gi = f - a.F;
        if (gi >= a.G || px >= (long)a.ohd * a.owd) return;
        const int y = (int)(px / a.owd), x = (int)(px - (long)y * a.owd);
        const int sy = nearest_src(y, a.Hd, a.ohd), sx = nearest_src(x, a.Wd, a.owd);
        const unsigned short v = a.depth[((size_t)gi * a.Hd + sy) * a.Wd + sx];
        a.depth_out[(size_t)gi * a.ohd * a.owd + (size_t)px] = (float)(short)v / 1000.0f;
    }
}

}  // namespace
}  // namespace pcrcg

using namespace pcrcg;

extern "C" {

int pcrcg_prepare_frames(const uint8_t* color, int F, int H, int W, int oh, int ow, float* color_out, const uint16_t* depth,
                         int G, int Hd, int Wd, int ohd, int owd, float* depth_out, void* stream) {
    constexpr int kMaxSide = 1 << 15;
    PCRCG_CHECK_ARG(F >= 0 && G >= 0 && F + G >= 1 && F + G <= 65535);
    PCRCG_CHECK_ARG(F == 0 || (color && color_out && H >= 1 && W >= 1 && oh >= 1 && ow >= 1 && H <= kMaxSide && W <= kMaxSide &&
                               oh <= kMaxSide && ow <= kMaxSide));
    PCRCG_CHECK_ARG(G == 0 || (depth && depth_out && Hd >= 1 && Wd >= 1 && ohd >= 1 && owd >= 1 && Hd <= kMaxSide &&
                               Wd <= kMaxSide && ohd <= kMaxSide && owd <= kMaxSide));
    FramesArgs a;
    a.color = color; a.color_out = color_out; a.depth = depth; a.depth_out = depth_out;
    a.F = F; a.H = H; a.W = W; a.oh = oh; a.ow = ow;
    a.G = G; a.Hd = Hd; a.Wd = Wd; a.ohd = ohd; a.owd = owd;
    const long pc = F ? (long)oh * ow : 0, pd = G ? (long)ohd * owd : 0;
    const long px = pc > pd ? pc : pd;
    hipLaunchKernelGGL(k_prepare_frames, dim3((unsigned)((px + 255) / 256), (unsigned)(F + G)), dim3(256), 0, as_stream(stream),
                       a);
    PCRCG_CHECK_LAUNCH();
    return PCRCG_OK;
}

}
