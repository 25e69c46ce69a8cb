// Internal launchers of finetune.hip (include/msig_ft.h).
#pragma once
#include "msig_dev.h"
#include "../../include/msig_ft.h"

// The folds of a head-epoch launch (msig_ft_multi after its checks; a single call is n = 1, slot 0).
struct FtFolds {
  int32_t n;
  int32_t slot[MSIG_MAX_FOLDS];
  int64_t stride;
  float lr[MSIG_MAX_FOLDS];
  int64_t step0[MSIG_MAX_FOLDS];
  uint64_t seed[MSIG_MAX_FOLDS];
};
int launch_head_epoch(const msig_ft_head& h, const FtFolds& ff, hipStream_t st);
// MSIG_WS_FEAT (B,128) of every fold of the launch -> out + z * out_stride_bytes
int launch_ft_feat_copy(const float* feat, float* out, int64_t out_stride_bytes, int B, const FoldCtx& fc, hipStream_t st);
