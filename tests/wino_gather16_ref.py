"""The 16-byte gather table of conv_wino4_kernel (csrc/wino_common.h: gather_decode16; csrc/conv_wino4.hip: the G16 form) restated in
plain Python, shared by test_wino_gather16_cpu.py and the rows of test_wino_gather16_gpu.py.  Nothing here imports the library.

R of one chunk: 4 channels x 18 rows x 40 floats, channel stride 768 floats (720 used), counted in float4 slots: 192 per channel (180
used), 10 per row.  Row float 3 + c holds patch column c (ox = x0 - 1 + c), so slot j of a row is the aligned global piece
ox = x0 - 4 + 4j .. x0 - 1 + 4j.  The 12 wave-instructions of a slot (64 float4 each) all belong to the four heavy waves (threads 0..255,
the waves with time to spare before the chunk barrier): thread tid requests slots tid, 256 + tid and 512 + tid; threads 256..511
request nothing."""
NT = 512
CK, TRH, RCOLS = 4, 18, 34          # channels per chunk, patch rows and columns with the halo
RS, PS, PSP = 40, 720, 768          # floats: row stride, used floats per channel, channel stride
RS4, PS4, PSP4 = RS // 4, PS // 4, PSP // 4
SLOTS = CK * PSP4                   # 768
HEAVY_THREADS = 256                 # the threads (waves 0-3) that carry the requests
ES = 256                            # slots between two requests of a thread


def requests(tid):
    """the request indices i of thread tid"""
    return (0, 1, 2) if tid < HEAVY_THREADS else ()


def decode_slot(e, y0, x0, H, W):
    """(byte offset inside the sample's chunk, or -1; mask bit) of float4 slot e for the patch whose first output pixel is (y0, x0)
    of an H x W image -- the arithmetic of gather_decode16, line by line"""
    ci = e // PSP4
    rem = e - PSP4 * ci
    r = rem // RS4
    j = rem - RS4 * r
    oy, ox4 = y0 - 1 + r, x0 - 4 + 4 * j
    valid = rem < PS4 and 0 <= oy < H and 0 <= ox4 < W
    return ((ci * H * W + oy * W + ox4) * 4 if valid else -1), (0 if valid else 1)


def table(y0, x0, H, W):
    """{(tid, i): byte offset} and {tid: mask} of one item, as the kernel's 512 threads write them"""
    offs, masks = {}, {}
    for tid in range(NT):
        m = 0
        for i in requests(tid):
            off, bit = decode_slot(tid + i * ES, y0, x0, H, W)
            offs[(tid, i)] = off
            m |= bit << i
        masks[tid] = m
    return offs, masks


def lds_image(offs):
    """R as the requests fill it: float index -> source float index inside the chunk (None = 0.0 from a failed range check).  A
    wave-instruction writes lane-linear: request i of wave w lands at byte (w + 4 i) * 1024 + lane * 16 of the slot."""
    R = {}
    for (tid, i), off in offs.items():
        wave, lane = tid >> 6, tid & 63
        byte = (wave + 4 * i) * 1024 + lane * 16
        assert byte % 16 == 0 and byte // 16 == tid + i * ES
        for k in range(4):
            assert byte // 4 + k not in R, "two requests write one LDS float"
            R[byte // 4 + k] = None if off < 0 else off // 4 + k
    return R
