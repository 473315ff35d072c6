// Argument block of the Winograd weight-gradient kernel (conv_wino_wgrad.hip), filled by idiff_conv2d_wgrad (conv_wgrad.hip).
#pragma once
#include "common.h"

namespace idiff_detail {

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

bool wino_wgrad_eligible(const WwArgs& a, int ks, int mode);
void wino_wgrad_geometry(int Cin, int Cout, int B, int Hout, int Wout, int* ncob, int* ncib, int* nsplit);
int launch_wino_wgrad(const WwArgs& a, int mode, hipStream_t st);

// conv_wino4_wgrad.hip: the F(4x4,3x3) form (normal and upsample mode; Hout % 4 == 0, Wout % 16 == 0, Cout % 64 == 0, Cin % 16 == 0); blocks of
// 64 co x 32 ci, same ws layout [nsplit][9][Cin][Cout]
bool wino4_wgrad_eligible(const WwArgs& a, int ks, int mode);
void wino4_wgrad_geometry(int Cin, int Cout, int B, int Hout, int Wout, int* ncob, int* ncib, int* nsplit);
int launch_wino4_wgrad(const WwArgs& a, hipStream_t st);

// conv_bf16_wgrad.hip: the bf16-operand weight gradient (idiff_conv_desc.operands == 1); same shapes as conv_bf16_eligible.  Its own
// workspace layout [B * K-blocks per sample][Cout][Cin][3][3] (bf16_wgrad_ws_floats) and its own ordered reduction into dw.
bool bf16_wgrad_eligible(const WwArgs& a, int ks, int mode);
long long bf16_wgrad_ws_floats(int Cin, int Cout, int B, int Hout, int Wout);
int launch_bf16_wgrad(const WwArgs& a, float* dw, int accumulate, hipStream_t st);

}  // namespace idiff_detail
