// Argument block of the Winograd weight-gradient kernel (conv_wino_wgrad.hip), filled by idiff_conv2d_wgrad (conv_wgrad.hip).
#pragma once
#include "conv_args.h"

namespace idiff_detail {

// The head that WwArgs below and conv_wgrad.hip's WgArgs share, src0 through ws
template <typename A>
inline void fill_wgrad_head(A& a, const idiff_conv_desc* d, const ConvShape& s, const float* dy, long long dybs, float* ws) {
    a.src0 = d->src0, a.src1 = d->src1, a.bs0 = d->src0_bstride, a.bs1 = d->src1_bstride;
    a.C0v = s.C0v, a.C1v = s.C1v, a.C0r = d->C0, a.Cin = s.Cin;
    a.B = d->B, a.Hin = d->Hin, a.Win = d->Win, a.Hout = s.Hout, a.Wout = s.Wout, a.Cout = d->Cout;
    a.pro_a = d->pro_a, a.pro_b = d->pro_b, a.dy = dy, a.dybs = dybs, a.ws = ws;
}

struct WwArgs {
    const float* src0;
    const float* src1;
    long long bs0, bs1;
    int C0v, C1v, C0r, Cin;
    int B, Hin, Win, Hout, Wout;
    int Cout;
    const float* pro_a;
    const float* pro_b;
    const float* dy;
    long long dybs;
    float* ws;  // [nsplit][9][Cin][Cout]
    int ncob, ncib, nsplit;
    int ups;  // F(4x4,3x3) form only: the input is the nearest x2 upsample of src0 (IDIFF_CONV_UPSAMPLE2)
};

// *_shape: "this shape could be mine", the part of *_eligible that the shape alone decides.  idiff_conv2d_wgrad_ws_floats sizes the
// workspace for every kernel that says so, so the one that is chosen cannot write past it.
bool wino_wgrad_shape(int ks, int Cout);
bool wino_wgrad_eligible(const WwArgs& a, int ks, int mode);
void wino_wgrad_geometry(int Cin, int Cout, int B, int Hout, int Wout, int* ncob, int* ncib, int* nsplit);
int launch_wino_wgrad(const WwArgs& a, int mode, hipStream_t st);

// conv_wino4_wgrad.hip: the F(4x4,3x3) form (normal and upsample mode; Hout % 4 == 0, Wout % 16 == 0, Cout % 64 == 0, Cin % 16 == 0); blocks of
// 64 co x 32 ci, same ws layout [nsplit][9][Cin][Cout]
bool wino4_wgrad_shape(int ks, int Cout, int Hout, int Wout);
bool wino4_wgrad_eligible(const WwArgs& a, int ks, int mode);
void wino4_wgrad_geometry(int Cin, int Cout, int B, int Hout, int Wout, int* ncob, int* ncib, int* nsplit);
int launch_wino4_wgrad(const WwArgs& a, hipStream_t st);

// conv_bf16_wgrad.hip: the bf16-operand weight gradient (idiff_conv_desc.operands == 1); same shapes as conv_bf16_eligible.  Its own
// workspace layout [B * K-blocks per sample][Cout][Cin][3][3] (bf16_wgrad_ws_floats) and its own ordered reduction into dw.
bool bf16_wgrad_eligible(const WwArgs& a, int ks, int mode);
long long bf16_wgrad_ws_floats(int Cin, int Cout, int B, int Hout, int Wout);
int launch_bf16_wgrad(const WwArgs& a, float* dw, int accumulate, hipStream_t st);

}  // namespace idiff_detail
