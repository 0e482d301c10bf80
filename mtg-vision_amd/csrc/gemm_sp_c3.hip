// LDS-DMA split GEMM, tile configuration 3: 4 x 1 waves, wave tile 32 x 64, block 128 x 64.
#define SP_CFG_ID 3
#include "gemm_sp_inst.h"
