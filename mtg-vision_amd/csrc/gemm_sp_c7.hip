// LDS-DMA split GEMM, tile configuration 7 (SP_CFG_N160): 4 x 1 waves, wave tile 32 x 160, block 128 x 160 - the window
// conv (A mode 5) for the detector heads' stacked first 3x3 convs (64 box + 64 class + 32 coefficient columns): one
// column tile, so no MFMA multiplies columns that do not exist and the input window is staged once.  One instance
// (SiLU, SP8 out, two-deep weight ring: gemm_sp_inst.h).
#define SP_CFG_ID 7
#include "gemm_sp_inst.h"
