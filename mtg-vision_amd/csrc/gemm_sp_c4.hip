// LDS-DMA split GEMM, tile configuration 4: 4 x 1 waves, wave tile 32 x 32, block 128 x 32.
#define SP_CFG_ID 4
#include "gemm_sp_inst.h"
