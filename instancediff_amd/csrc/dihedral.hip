// Flips and transpositions of image rows (include/idiff.h, idiff_dihedral_rows): the geometric self-ensemble of driftSDE turns every
// member's input before the chain and its sample back after it.  A pure permutation of 32-bit words: nothing here does arithmetic on
// the values, so signed zeros and NaN payloads pass through.
//
// One kernel, 256 threads, one 64x64 tile of one (row, channel) plane of the OUTPUT per block; the code is uniform per block.
//   * codes without the transposition: no LDS.  Lane (i, j) = (tid >> 4, tid & 15) moves the 16-byte piece j of tile rows i, i + 16,
//     i + 32, i + 48: one load at the mirrored position, its four words reversed when W is flipped, one store.  16 lanes cover 256
//     contiguous bytes on both sides.
//   * codes with the transposition (H == W): the source tile goes through LDS as tile[a][b] = out-tile(y0 + b, x0 + a), pitch 65
//     dwords.  Loads are 16 bytes along the source's W (the b axis; reversed when H is flipped, since the flips follow the
//     transposition), stores 16 bytes along the output's W (the a axis).  With the pitch odd, bank = (a + b) mod 64: a wave's 64 dword
//     writes (4 values of a, 16 of b4, fixed word) and its 64 column reads (16 values of a4, 4 of b, fixed word) each hit 64 banks.
// Edge tiles are guarded per 16-byte piece: W % 4 == 0 (and H == W where it matters), so a piece never straddles an edge.
#include "common.h"

namespace {

constexpr int DT = 64;        // tile edge
constexpr int DPITCH = 65;    // LDS row pitch in dwords

__device__ __forceinline__ uint4 rev4(uint4 v) { return make_uint4(v.w, v.z, v.y, v.x); }

__global__ __launch_bounds__(256) void dihedral_rows_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, int C, int H, int W,
                                                            int in_rep, int S, int period, uint32_t codes, int tiles_x) {
    __shared__ uint32_t tile[DT * DPITCH];
    const int r = blockIdx.z, c = blockIdx.y;
    const uint32_t k = (codes >> (3 * ((r % S) % period))) & 7u;
    const bool tr = k & 1u, fh = k & 2u, fw = k & 4u;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int y0 = ty * DT, x0 = tx * DT;
    const long long plane = (long long)H * W;
    const uint32_t* src = in + ((long long)(r / in_rep) * C + c) * plane;
    uint32_t* dst = out + ((long long)r * C + c) * plane;
    const int i = threadIdx.x >> 4, j4 = (threadIdx.x & 15) * 4;

    if (!tr) {
        const int x = x0 + j4;
        if (x >= W) return;
        const int xs = fw ? W - 4 - x : x;
#pragma unroll
        for (int q = 0; q < DT; q += 16) {
            const int y = y0 + i + q;
            if (y < H) {
                const int ys = fh ? H - 1 - y : y;
                uint4 v = *reinterpret_cast<const uint4*>(src + (long long)ys * W + xs);
                if (fw) v = rev4(v);
                *reinterpret_cast<uint4*>(dst + (long long)y * W + x) = v;
            }
        }
        return;
    }

    // tile[a][b] = src[x1(x0 + a)][y1(y0 + b)]: source row from the output's x, source column from the output's y
    {
        const int y = y0 + j4;  // output rows y .. y + 3 = the four words of this piece
        if (y < H) {
            const int cs = fh ? H - 4 - y : y;
#pragma unroll
            for (int q = 0; q < DT; q += 16) {
                const int a = i + q, x = x0 + a;
                if (x < W) {
                    const int rs = fw ? W - 1 - x : x;
                    uint4 v = *reinterpret_cast<const uint4*>(src + (long long)rs * W + cs);
                    if (fh) v = rev4(v);
                    uint32_t* t = tile + a * DPITCH + j4;
                    t[0] = v.x, t[1] = v.y, t[2] = v.z, t[3] = v.w;
                }
            }
        }
    }
    __syncthreads();
    {
        const int x = x0 + j4;
        if (x >= W) return;
#pragma unroll
        for (int q = 0; q < DT; q += 16) {
            const int b = i + q, y = y0 + b;
            if (y < H) {
                const uint32_t* t = tile + j4 * DPITCH + b;
                const uint4 v = make_uint4(t[0], t[DPITCH], t[2 * DPITCH], t[3 * DPITCH]);
                *reinterpret_cast<uint4*>(dst + (long long)y * W + x) = v;
            }
        }
    }
}

}  // namespace

extern "C" int idiff_dihedral_rows(const float* in, float* out, int R, int C, int H, int W, int in_rep, int S, int period, uint32_t codes,
                                   idiff_stream_t stream) {
    IDIFF_CHECK_ARG(in && out, "dihedral_rows: null operand");
    IDIFF_CHECK_ARG(period >= 1 && period <= 8 && S >= 1 && in_rep >= 1 && R >= 1 && R % in_rep == 0 && C >= 1 && H >= 1 && W >= 4,
                    "dihedral_rows: bad sizes (R=%d C=%d H=%d W=%d in_rep=%d S=%d period=%d)", R, C, H, W, in_rep, S, period);
    IDIFF_CHECK_ARG(W % 4 == 0, "dihedral_rows: W = %d is not a multiple of 4", W);
    bool transposes = false;
    for (int p = 0; p < period; ++p) transposes |= (codes >> (3 * p)) & 1u;
    IDIFF_CHECK_ARG(!transposes || H == W, "dihedral_rows: a transposing code needs a square image, got %d x %d", H, W);
    IDIFF_CHECK_ARG(((uintptr_t)in & 15) == 0 && ((uintptr_t)out & 15) == 0, "dihedral_rows: operands must be 16-byte aligned");
    const long long tiles_x = (W + DT - 1) / DT, tiles = tiles_x * ((H + DT - 1) / DT);
    // the grid: x = tiles of a plane, y = channels, z = rows
    IDIFF_CHECK_ARG(R <= 65535 && C <= 65535 && tiles <= 0x7fffffffLL, "dihedral_rows: R = %d / C = %d exceed 65535 (the grid's row and channel axes)",
                    R, C);
    const unsigned long long plane_bytes = 4ull * (unsigned long long)H * (unsigned long long)W * (unsigned long long)C;
    const uintptr_t in0 = (uintptr_t)in, in1 = in0 + plane_bytes * (unsigned long long)(R / in_rep);
    const uintptr_t out0 = (uintptr_t)out, out1 = out0 + plane_bytes * (unsigned long long)R;
    IDIFF_CHECK_ARG(in1 <= out0 || out1 <= in0, "dihedral_rows: in and out overlap");
    hipLaunchKernelGGL(dihedral_rows_kernel, dim3((unsigned)tiles, (unsigned)C, (unsigned)R), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const uint32_t*>(in), reinterpret_cast<uint32_t*>(out), C, H, W, in_rep, S, period, codes, (int)tiles_x);
    IDIFF_CHECK_LAUNCH("dihedral_rows");
    return IDIFF_OK;
}
