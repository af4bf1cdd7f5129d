"""Names of the GEMM / convolution kernels' ``variant`` bits (``csrc/gemm.h`` kVar*).

The one Python definition of each; ``ops/gemm.py`` and ``ops/conv.py`` re-export the
ones they are known by (``gemm.PP``, ``conv.T64``).  The values are part of the tuner's
choice names (``native:2048:6``), of ``P2PFL_GEMM_VARIANT`` and of the committed
profiles.  The extension exports the C++ values as ``gemm_variant_bits``
(``tests/test_gpu_gemm.py`` compares the two); this module imports without it.
"""

SETPRIO = 1  # s_setprio around the core kernel's MFMA clusters
A_PANEL = 2  # consecutive tiles share an A panel (default: a B panel)
NO_XCD_REMAP = 4  # workgroup ids as dispatched
SINGLE_BUF = 8  # 128 x 128 tile on one LDS buffer, 4 workgroups per CU
PROBE_NO_STORE = 16  # core kernel timing probes: wrong results on purpose
PROBE_NO_KLOOP = 32
TILE256 = 64  # 256 x 256 tile on the core pipeline
PROBE_NO_DMA = 128
LEGACY_ORDER = 256  # plain panel tile order instead of grouped
PREFETCH_SHIFT = 9  # bits 9-10: where the double buffer's prefetch is issued
PREFETCH_MASK = 3 << 9
PP = 2048  # the ping-pong 256 x 256 pipeline (csrc/gemm_pp.hip)
RING4 = 4096  # 128 x 128 tile on a 4-stage LDS ring, one workgroup per CU
T64 = 1 << 14  # convolutions only: 64 x 64 output tiles
PP_M16 = 1 << 16  # with PP: the same pipeline on v_mfma_f32_16x16x32_bf16
PP_SK = 1 << 17  # with PP: stream-K schedule, ``splits`` = grid size
PP_N128 = 1 << 21  # with PP: the 256 x 128 output tile (150 whole tiles for the N = 768 products)
PP_REFUSED = (15 << 12) | (7 << 18)  # with PP: bits that select nothing; the binding refuses them
