"""The key-split table of the ScoreMapModule cross-attention (smm_split in csrc/attention.hip), shared by the GPU rows of
test_step_kernels_gpu.py and their CPU mirror test_step_split_cpu.py (idiff_smm_xattn_ws_floats is host-only).

The rule: nkb = ceil(N / 32) key blocks; k = nkb / 32 blocks per split, floored to 2, capped at 64 and at nkb; nsplit = ceil(nkb / k).
Cm = 72 takes smm_xattn_w_kernel<72> when k >= 4, else smm_xattn_kernel<18>; 136 -> <34>; 256 -> <64>."""

SPLIT_ROWS = [
    # id, Cm, (Nq, heads), B, N, expected nsplit, expected kps, scale of the last split's keys (so that they carry weight)
    ("xattn-Cm256-rows1-nkb1-N4", 256, (1, 1), 1, 4, 1, 1, 1.0),
    ("xattn-Cm72-rows20-nkb1-N32-k18", 72, (5, 4), 2, 32, 1, 1, 1.0),
    ("xattn-Cm136-rows32-N36-ragged-block-k-capped-by-nkb", 136, (8, 4), 2, 36, 1, 2, 1.0),
    ("xattn-Cm256-rows32-N1024-k-floored-to-2", 256, (8, 4), 1, 1024, 16, 2, 1.0),
    ("xattn-Cm72-rows20-N3072-kps3-k18", 72, (5, 4), 2, 3072, 32, 3, 1.0),
    ("xattn-Cm72-rows20-N4064-kps3-last-nkb127-k18", 72, (5, 4), 1, 4064, 43, 3, 1.0),
    ("xattn-Cm72-rows20-N4096-kps4-wform", 72, (5, 4), 2, 4096, 32, 4, 1.0),
    ("xattn-Cm72-rows32-N4132-kps4-wform-ragged-split-ragged-block", 72, (8, 4), 1, 4132, 33, 4, 2.0),
    ("xattn-Cm136-rows1-N4132-ragged-split-ragged-block", 136, (1, 1), 2, 4132, 33, 4, 2.0),
    ("xattn-Cm256-rows20-N131232-k-capped-at-64-short-last-split", 256, (5, 4), 1, 131072 + 32 * 5, 65, 64, 3.0),
    ("xattn-Cm72-rows32-N131204-k-capped-at-64-wform-ragged-block", 72, (8, 4), 1, 131072 + 32 * 4 + 4, 65, 64, 3.0),
]


def split_rule(N):
    """(nsplit, kps) as the comment above states the rule -- written from the text, not from the library"""
    nkb = -(-N // 32)
    k = min(max(nkb // 32, 2), 64, nkb)
    return -(-nkb // k), k


def witnessed_nsplit(lib, B, Nq, heads, Cm, N):
    return lib.idiff_smm_xattn_ws_floats(B, Nq, heads, Cm, N) // (B * (Cm + 2) * 32)
