#!/bin/bash
# Negative controls of the parity gate (run on the GPU box, from the repository root; libraries built beforehand by
#   for k in 1 2 3 4 5 9; do make -C multimodalsignal_amd/csrc negctl NEGCTL=$k; done   -> multimodalsignal_amd/csrc/build/ ).
# Each library drops ONE cross term of the split products in ONE class of contractions (msig_dev.h CT_*): split-bf16 without a1 * b1
# (2^-16 relative per product), two-piece fp16 without a1 * b0 (2^-11).  1 backward recurrence, 2 dX, 3 dW, 4 forward recurrence,
# 5 forward projection, 9 all of them.  Every selected case must FAIL against every control and PASS against the product library;
# the script prints per-case verdicts and EXITS NON-ZERO when a control passes a case or the product fails one.
# tools/negative_controls.sh regime [OUT] [LIBRARY ...]: the controls of the TRAINED-LIKE regimes instead (libraries built by
#   for k in 1 2 3 4; do make -C multimodalsignal_amd/csrc negctl REGIME=$k; done ).  Each is one slip that is invisible near
# initialisation (msig_dev.h MSIG_NEGCTL_REGIME): 1 the recovery of n without its floor, 2 sigmoid as e^x / (1 + e^x), 3 BatchNorm's
# scale from |gamma|, 4 log-sum-exp without the row maximum.  Per library: one pass of tests/test_trained_regimes_gpu.py (must FAIL,
# in the regime named below) and one of the OLD selection, tests/test_parity_gpu.py -k "golden_case or ws6" (recorded: did the suite
# notice before?); `product` runs the new file only (the old selection against it is part of the ordinary tier).  Every pass has its
# own time limit and the script stops at the first abnormal exit (anything but pytest's 0 / 1).  LIBRARY: product 1 2 3 4 (default
# all); sections are kept per library beside OUT and OUT is assembled from those present, so the passes may be spread over calls.
# tools/negative_controls.sh range [OUT] [LIBRARY ...]: the controls of the CHANNEL / CLASS RANGE (libraries built by
#   for k in 1 2 3; do make -C multimodalsignal_amd/csrc negctl RANGE=$k; done ).  Each is one in-bounds slip in code that only
# C = 9..15 or K > 8 reach (msig_dev.h MSIG_NEGCTL_RANGE): 1 conv1_fwd<0> without the zero fill of its padded taps, 2 conv1_bwd<0>
# without its partial last column block, 3 dW3 in two of its four register slots.  Per library: one pass of
# tests/test_channel_class_range_gpu.py (must FAIL at least one case; the product must pass every case) and one of the OLD selection,
# tests/test_parity_gpu.py -k "golden_case or ws6" (recorded: did the suite notice before?), with the time limits, the stop at the
# first abnormal exit and the per-library sections of the regime mode.  LIBRARY: product 1 2 3 (default all).
# tools/negative_controls.sh input [OUT] [LIBRARY ...]: the controls of the INPUT regimes (libraries built by
#   for k in 1 2; do make -C multimodalsignal_amd/csrc negctl INPUT=$k; done ).  Each is one slip that no unit-scale, nearly centred
# input can see (msig_dev.h MSIG_NEGCTL_INPUT): 1 the conv kernels' BatchNorm sums accumulated unshifted and reduced in fp32, 2 eps added
# outside bn_finalize's square root.  Per library: one pass of tests/test_input_regimes_gpu.py with the AdaBN gate of
# tests/test_adapt_gpu.py (must FAIL, in the regime named below) and one of the OLD selection, tests/test_parity_gpu.py -k "golden_case or
# ws6" (recorded: did the suite notice before?  control 1 is the arithmetic those cases always ran and must pass them), with the time
# limits, the stop at the first abnormal exit and the per-library sections of the regime mode.  LIBRARY: product 1 2 (default all).
# tools/negative_controls.sh length [OUT] [LIBRARY ...]: the controls of the WINDOW LENGTHS (libraries built by
#   for k in 1 2 3; do make -C multimodalsignal_amd/csrc negctl LENGTH=$k; done ).  Each is one in-bounds slip in a guard that only an
# unaligned window with more than one chunk reaches (msig_dev.h MSIG_NEGCTL_LENGTH): 1 stage_x_chunk's scalar branch reads the window's
# last sample as padding in an item with t0 > 0, 2 conv1_bwd<CT > 0>'s non-prefetch staging at T % 8 == 4 zeroes position L1 - 1,
# 3 conv1_bwd_dx's position-wise staging zeroes position L1 - 1 in an item with u0 > 0.  Per library: one pass of
# tests/test_window_lengths_gpu.py (must FAIL at least one case; the product must pass every case) and one of the cases that ran
# unaligned lengths BEFORE — T = 137 and 250 of tests/test_parity_gpu.py, tests/test_input_grad_gpu.py, the T = 137, 250 and 511 cases
# of tests/test_channel_class_range_gpu.py and the input-gradient cases (T = 511) of tests/test_input_regimes_gpu.py — which must PASS:
# that pass is the evidence that the suite had the gap.  Time limits, the stop at the first abnormal exit and the per-library
# sections as in the regime mode.  LIBRARY: product 1 2 3 (default all).
# tools/negative_controls.sh supcon [OUT] [LIBRARY ...]: the control of the SUPERVISED CONTRASTIVE term (library
# built by  make -C multimodalsignal_amd/csrc negctl SUPCON=1 ): sc_grad_kernel without the transposed term C_ji (msig_dev.h
# MSIG_NEGCTL_SUPCON).  Per library: one pass of the `apply` parity cases of tests/test_supcon_gpu.py — the product must pass every
# case, the control must FAIL every case whose gradient is not identically zero (B = 1 has no anchor and writes nothing; at B = 2 an
# anchor has one positive and nothing else in A(i), so C_ij = 1 - 1 = 0 whatever the features are).  Time limit, the stop at the
# first abnormal exit and the per-library sections as in the regime mode.  LIBRARY: product 1 (default both).
# tools/negative_controls.sh stage2 [OUT] [LIBRARY ...]: the control of the STAGE-2 regimes (DESIGN.md "Stage-2 regimes"; library built by
#   make -C multimodalsignal_amd/csrc negctl STAGE2=1 ): bn_batch_sums takes the unshifted fp32 sums for every conv2 channel (msig_dev.h
# MSIG_NEGCTL_STAGE2) — the arithmetic stage 2 had before pool1_conv2_fwd_kernel carried shifted sums.  Per library: one pass of
# tests/test_stage2_regimes_gpu.py (the product must pass every case; the control must FAIL the conv2_offcentre cases at one, two and
# four work items) and one of the files that held the regimes BEFORE, tests/test_trained_regimes_gpu.py and
# tests/test_input_regimes_gpu.py, which must PASS against the control: it is the arithmetic they always ran, and that pass is the
# evidence that the suite had the gap.  Time limits, the stop at the first abnormal exit and the per-library sections as in the regime
# mode.  LIBRARY: product 1 (default both).
# tools/negative_controls.sh tent [OUT] [LIBRARY ...]: the control of the ENTROPY-MINIMISATION objective (library
# built by  make -C multimodalsignal_amd/csrc negctl TENT=1 ): tt_objective_kernel's gradient without H_b, -p lp alone (tta.hip
# MSIG_NEGCTL_TENT).  Per library: one pass of the objective's parity cases of tests/test_entropy_adapt_gpu.py — the product must pass
# every case, the control must FAIL every case (every case holds a row whose entropy is of order 1: uniform rows, and saturated rows
# with their peak twice).  Time limit, the stop at the first abnormal exit and the per-library sections as in the regime mode.
# LIBRARY: product 1 (default both).
# tools/negative_controls.sh mixed [OUT] [LIBRARY ...]: the control of the MIXED-RATE push (library built by
#   make -C multimodalsignal_amd/csrc negctl MIXED=1 ): mx_lv_push_kernel reads tail row (j + 1) % tail_rows for raw row j (mixed.hip
# MSIG_NEGCTL_MIXED), in bounds by construction.  Per library: one pass of the single-group test and of the chunking cases of
# tests/test_mixed_rate_gpu.py — the product must pass every case, the control must FAIL every one (each pushes chunks whose first
# outputs reach behind the chunk).  Time limit, the stop at the first abnormal exit and the per-library sections as in the regime mode.
# LIBRARY: product 1 (default both).
# tools/negative_controls.sh batch [OUT] [LIBRARY ...]: the controls of the BATCH SIZES (DESIGN.md "Batch sizes"; libraries built by
#   for k in 1 2 3 4; do make -C multimodalsignal_amd/csrc negctl BATCH=$k; done ).  Each is one in-bounds, arithmetic-only slip in a guard
# on the batch size (msig_dev.h MSIG_NEGCTL_BATCH): 1 the latency form's backward recurrence keeps the gate gradients of padding rows in
# the second half of a ragged tile, 2 the CrossEntropy row loops start their second pass one row late, 3 head_bwd's group loop skips a
# one-row last group beyond its 128-workgroup grid, 4 a workgroup of the capped dW grid stops after its 8 units.  Per library: one pass
# of tests/test_batch_sizes_gpu.py (must FAIL at least one case; the product must pass every case) and one of the files the suite had
# BEFORE that could notice such a slip (OLDF below), recorded: did the suite notice before?  OLDF is NOT the whole -m gpu suite, which
# is too long to repeat per library: it is every file that holds the HIP path to the oracle through gpu_common.run_case (the
# bit-for-bit tests of tests/test_parity_gpu.py among them) and the files that hold the head, the CrossEntropy kernels and the train
# step to a reference of their own (the cnn_gru kind, class weights, soft targets, the head's golden vectors, the step dispatch); the
# files left out drive monitoring, preprocessing, the LOSO analyses and the optional step terms, whose references are the same
# library's other entry points.  The log's header repeats this restriction.  Controls 2 and 3 are EXPECTED to be noticed there — the
# CrossEntropy loops and head_bwd's second round have no side the old cases miss (B = 3100 and 4100 run four and five passes against the
# oracle; tests/test_class_weights_gpu.py and tests/test_soft_targets_gpu.py hold the step to an fp64 reference at B = 2049, a last group
# of one row) — and the script says so: they show that the new cases see such slips too, not that the suite had a gap.  Controls 1 and 4
# must pass the old files: that pass is the evidence that the suite had the gap.  Time limits, the
# stop at the first abnormal exit and the per-library sections as in the regime mode.  LIBRARY: product 1 2 3 4 (default all).
if [ "$1" = batch ]; then
  OUT=${2:-batch_negctl_out/batch_negative_control.log}
  D=$(dirname "$OUT")
  shift; shift
  LIBS=${*:-product 1 2 3 4}
  OLDF='tests/test_parity_gpu.py tests/test_trained_regimes_gpu.py tests/test_input_regimes_gpu.py tests/test_window_lengths_gpu.py tests/test_channel_class_range_gpu.py tests/test_stage2_regimes_gpu.py tests/test_cnngru_gpu.py tests/test_class_weights_gpu.py tests/test_soft_targets_gpu.py tests/test_head_mlp_golden_gpu.py tests/test_step_dispatch_gpu.py'
  NEW=tests/test_batch_sizes_gpu.py
  mkdir -p "$D"
  bad=0
  for k in $LIBS; do
    if [ "$k" = product ]; then lib=$PWD/multimodalsignal_amd/libmsig_hip.so; else lib=$PWD/multimodalsignal_amd/csrc/build/libmsig_hip_batch$k.so; fi
    sec=$D/batch_negctl_section_$k.log
    [ -f "$lib" ] || { echo "## library: $(basename $lib): missing" > $sec; bad=1; continue; }
    MSIG_LIB=$lib timeout -k 10 480 python -m pytest $NEW -q -rA -p no:cacheprovider > $D/batch_negctl_${k}_new.txt 2>&1; rc=$?
    echo "## library: $(basename $lib)" > $sec
    echo "# new file, $NEW (exit $rc):   $(tail -1 $D/batch_negctl_${k}_new.txt)" >> $sec
    if [ "$k" = product ]; then grep -E "^(PASSED|FAILED) " $D/batch_negctl_${k}_new.txt | sed 's/ - .*//' | sort >> $sec
    else grep -E "^FAILED " $D/batch_negctl_${k}_new.txt | sed 's/ - .*//' | sort >> $sec; fi
    if [ $rc != 0 ] && [ $rc != 1 ]; then echo "!! abnormal exit $rc: stopped here" >> $sec; bad=2; break; fi
    nfail=$(grep -c "^FAILED " $D/batch_negctl_${k}_new.txt)
    if [ "$k" = product ]; then
      [ $rc = 0 ] || { echo "!! the product library must pass the new file" >> $sec; bad=1; }
      continue
    fi
    if [ "$nfail" -gt 0 ]; then echo "# verdict: control $k FAILS $nfail new cases" >> $sec
    else echo "!! control $k fails no new case: the new file does not catch it" >> $sec; bad=1; fi
    MSIG_LIB=$lib timeout -k 10 600 python -m pytest $OLDF -q -rA -p no:cacheprovider > $D/batch_negctl_${k}_old.txt 2>&1; rc=$?
    echo "# the files the suite had, $OLDF (exit $rc):   $(tail -1 $D/batch_negctl_${k}_old.txt)" >> $sec
    grep -E "^FAILED " $D/batch_negctl_${k}_old.txt | sed 's/ - .*//' | sort >> $sec
    if [ $rc != 0 ] && [ $rc != 1 ]; then echo "!! abnormal exit $rc: stopped here" >> $sec; bad=2; break; fi
    if [ $rc = 0 ]; then echo "# verdict: the files the suite had do NOT notice control $k" >> $sec
    elif [ "$k" = 2 ]; then echo "# verdict: the files the suite had NOTICE control 2, as expected: it is no evidence of a gap (the new cases at B = 1025 .. 2048 hold loss_finalize to the oracle; the loops themselves were covered)" >> $sec
    elif [ "$k" = 3 ]; then echo "# verdict: the files the suite had NOTICE control 3, as expected: it is no evidence of a gap (B = 2049 of the class-weight and soft-target steps has a one-row last group in head_bwd's second round)" >> $sec
    else echo "!! the files the suite had notice control $k: the slip is not confined to the new batch sizes" >> $sec; bad=1; fi
  done
  echo "# tools/negative_controls.sh batch: $NEW and the files the suite had against libmsig_hip_batch<k>.so (make negctl BATCH=k)" > "$OUT"
  echo "# 'the files the suite had' are the parity, head, CrossEntropy and train-step files of the suite before this table, NOT the whole -m gpu suite (too long to repeat per library): a verdict 'do NOT notice' is about these files" >> "$OUT"
  for k in product 1 2 3 4; do [ -f $D/batch_negctl_section_$k.log ] && cat $D/batch_negctl_section_$k.log >> "$OUT"; done
  tail -n +1 "$OUT"
  exit $bad
fi
if [ "$1" = tent ]; then
  OUT=${2:-tent_negctl_out/entropy_adapt_negative_control.log}
  D=$(dirname "$OUT")
  shift; shift
  LIBS=${*:-product 1}
  NEW=tests/test_entropy_adapt_gpu.py::test_objective_against_the_reference
  mkdir -p "$D"
  bad=0
  for k in $LIBS; do
    if [ "$k" = product ]; then lib=$PWD/multimodalsignal_amd/libmsig_hip.so; else lib=$PWD/multimodalsignal_amd/csrc/build/libmsig_hip_tent$k.so; fi
    sec=$D/tent_negctl_section_$k.log
    [ -f "$lib" ] || { echo "## library: $(basename $lib): missing" > $sec; bad=1; continue; }
    MSIG_LIB=$lib timeout -k 10 420 python -m pytest $NEW -q -rA -p no:cacheprovider > $D/tent_negctl_${k}.txt 2>&1; rc=$?
    echo "## library: $(basename $lib)" > $sec
    echo "# $NEW (exit $rc):   $(tail -1 $D/tent_negctl_${k}.txt)" >> $sec
    grep -E "^(PASSED|FAILED) " $D/tent_negctl_${k}.txt | sed 's/ - .*//' | sort >> $sec
    if [ $rc != 0 ] && [ $rc != 1 ]; then echo "!! abnormal exit $rc: stopped here" >> $sec; bad=2; break; fi
    npass=$(grep -c "^PASSED " $D/tent_negctl_${k}.txt)
    nfail=$(grep -c "^FAILED " $D/tent_negctl_${k}.txt)
    if [ "$k" = product ]; then
      [ $rc = 0 ] && [ "$nfail" = 0 ] && [ "$npass" -gt 0 ] || { echo "!! the product library must pass every case" >> $sec; bad=1; }
      continue
    fi
    if [ "$npass" = 0 ] && [ "$nfail" -gt 0 ]; then echo "# verdict: control $k FAILS all $nfail cases" >> $sec
    else echo "!! control $k passes $npass cases: the gate does not catch it there" >> $sec; bad=1; fi
  done
  echo "# tools/negative_controls.sh tent: $NEW against libmsig_hip_tent1.so (make negctl TENT=1)" > "$OUT"
  for k in product 1; do [ -f $D/tent_negctl_section_$k.log ] && cat $D/tent_negctl_section_$k.log >> "$OUT"; done
  tail -n +1 "$OUT"
  exit $bad
fi
if [ "$1" = stage2 ]; then
  OUT=${2:-stage2_negctl_out/stage2_negative_control.log}
  D=$(dirname "$OUT")
  shift; shift
  LIBS=${*:-product 1}
  NEW=tests/test_stage2_regimes_gpu.py
  OLDF='tests/test_trained_regimes_gpu.py tests/test_input_regimes_gpu.py'
  mkdir -p "$D"
  bad=0
  for k in $LIBS; do
    if [ "$k" = product ]; then lib=$PWD/multimodalsignal_amd/libmsig_hip.so; else lib=$PWD/multimodalsignal_amd/csrc/build/libmsig_hip_stage2$k.so; fi
    sec=$D/stage2_negctl_section_$k.log
    [ -f "$lib" ] || { echo "## library: $(basename $lib): missing" > $sec; bad=1; continue; }
    MSIG_LIB=$lib timeout -k 10 420 python -m pytest $NEW -q -rA -p no:cacheprovider > $D/stage2_negctl_${k}_new.txt 2>&1; rc=$?
    echo "## library: $(basename $lib)" > $sec
    echo "# new file, $NEW (exit $rc):   $(tail -1 $D/stage2_negctl_${k}_new.txt)" >> $sec
    grep -E "^(PASSED|FAILED) " $D/stage2_negctl_${k}_new.txt | sed 's/ - .*//' | sort >> $sec
    if [ $rc != 0 ] && [ $rc != 1 ]; then echo "!! abnormal exit $rc: stopped here" >> $sec; bad=2; break; fi
    nfail=$(grep -c "^FAILED " $D/stage2_negctl_${k}_new.txt)
    if [ "$k" = product ]; then
      [ $rc = 0 ] || { echo "!! the product library must pass the new file" >> $sec; bad=1; }
      continue
    fi
    nwant=$(grep "^FAILED " $D/stage2_negctl_${k}_new.txt | grep -cE "conv2_offcentre-(1-6|2-6|4-3)-2-256")
    if [ "$nwant" = 6 ]; then echo "# verdict: control $k FAILS $nfail new cases, all 6 conv2_offcentre cases at 1, 2 and 4 work items among them" >> $sec
    else echo "!! control $k fails $nwant of the 6 conv2_offcentre cases at 1, 2 and 4 work items ($nfail failures in all)" >> $sec; bad=1; fi
    MSIG_LIB=$lib timeout -k 10 600 python -m pytest $OLDF -q -rA -p no:cacheprovider > $D/stage2_negctl_${k}_old.txt 2>&1; rc=$?
    echo "# the regime files the suite had, $OLDF (exit $rc):   $(tail -1 $D/stage2_negctl_${k}_old.txt)" >> $sec
    grep -E "^FAILED " $D/stage2_negctl_${k}_old.txt | sed 's/ - .*//' | sort >> $sec
    if [ $rc != 0 ] && [ $rc != 1 ]; then echo "!! abnormal exit $rc: stopped here" >> $sec; bad=2; break; fi
    if [ $rc = 0 ]; then echo "# verdict: the regime files the suite had do NOT notice control $k" >> $sec
    else echo "!! the regime files the suite had notice control $k: it is the arithmetic they always ran and must pass them" >> $sec; bad=1; fi
  done
  echo "# tools/negative_controls.sh stage2: $NEW and $OLDF against libmsig_hip_stage21.so (make negctl STAGE2=1)" > "$OUT"
  for k in product 1; do [ -f $D/stage2_negctl_section_$k.log ] && cat $D/stage2_negctl_section_$k.log >> "$OUT"; done
  tail -n +1 "$OUT"
  exit $bad
fi
if [ "$1" = mixed ]; then
  OUT=${2:-mixed_negctl_out/mixed_negative_control.log}
  D=$(dirname "$OUT")
  shift; shift
  LIBS=${*:-product 1}
  NEW="tests/test_mixed_rate_gpu.py::test_one_group_of_all_columns_is_the_single_rate_call tests/test_mixed_rate_gpu.py::test_every_way_of_chunking_gives_the_offline_bits"
  mkdir -p "$D"
  bad=0
  for k in $LIBS; do
    if [ "$k" = product ]; then lib=$PWD/multimodalsignal_amd/libmsig_hip.so; else lib=$PWD/multimodalsignal_amd/csrc/build/libmsig_hip_mixed$k.so; fi
    sec=$D/mixed_negctl_section_$k.log
    [ -f "$lib" ] || { echo "## library: $(basename $lib): missing" > $sec; bad=1; continue; }
    MSIG_LIB=$lib timeout -k 10 300 python -m pytest $NEW -q -rA -p no:cacheprovider > $D/mixed_negctl_${k}.txt 2>&1; rc=$?
    echo "## library: $(basename $lib)" > $sec
    echo "# $NEW (exit $rc):   $(tail -1 $D/mixed_negctl_${k}.txt)" >> $sec
    grep -E "^(PASSED|FAILED) " $D/mixed_negctl_${k}.txt | sed 's/ - .*//' | sort >> $sec
    if [ $rc != 0 ] && [ $rc != 1 ]; then echo "!! abnormal exit $rc: stopped here" >> $sec; bad=2; break; fi
    if [ "$k" = product ]; then
      [ $rc = 0 ] || { echo "!! the product library must pass every case" >> $sec; bad=1; }
      continue
    fi
    npass=$(grep -c "^PASSED " $D/mixed_negctl_${k}.txt)
    nfail=$(grep -c "^FAILED " $D/mixed_negctl_${k}.txt)
    if [ "$npass" = 0 ] && [ "$nfail" -gt 0 ]; then echo "# verdict: control $k FAILS all $nfail cases" >> $sec
    else echo "!! control $k passes $npass cases: the tests do not catch it there" >> $sec; bad=1; fi
  done
  echo "# tools/negative_controls.sh mixed: the single-group and chunking cases of tests/test_mixed_rate_gpu.py against libmsig_hip_mixed1.so (make negctl MIXED=1)" > "$OUT"
  for k in product 1; do [ -f $D/mixed_negctl_section_$k.log ] && cat $D/mixed_negctl_section_$k.log >> "$OUT"; done
  tail -n +1 "$OUT"
  exit $bad
fi
if [ "$1" = supcon ]; then
  OUT=${2:-supcon_negctl_out/supcon_negative_control.log}
  D=$(dirname "$OUT")
  shift; shift
  LIBS=${*:-product 1}
  NEW=tests/test_supcon_gpu.py::test_apply_matches_the_fp64_restatement
  mkdir -p "$D"
  bad=0
  for k in $LIBS; do
    if [ "$k" = product ]; then lib=$PWD/multimodalsignal_amd/libmsig_hip.so; else lib=$PWD/multimodalsignal_amd/csrc/build/libmsig_hip_supcon$k.so; fi
    sec=$D/supcon_negctl_section_$k.log
    [ -f "$lib" ] || { echo "## library: $(basename $lib): missing" > $sec; bad=1; continue; }
    MSIG_LIB=$lib timeout -k 10 420 python -m pytest $NEW -q -rA -p no:cacheprovider > $D/supcon_negctl_${k}.txt 2>&1; rc=$?
    echo "## library: $(basename $lib)" > $sec
    echo "# $NEW (exit $rc):   $(tail -1 $D/supcon_negctl_${k}.txt)" >> $sec
    grep -E "^(PASSED|FAILED) " $D/supcon_negctl_${k}.txt | sed 's/ - .*//' | sort >> $sec
    if [ $rc != 0 ] && [ $rc != 1 ]; then echo "!! abnormal exit $rc: stopped here" >> $sec; bad=2; break; fi
    if [ "$k" = product ]; then
      [ $rc = 0 ] || { echo "!! the product library must pass every case" >> $sec; bad=1; }
      continue
    fi
    npass=$(grep -E "^PASSED " $D/supcon_negctl_${k}.txt | grep -vc "\[[12]-")
    nfail=$(grep -c "^FAILED " $D/supcon_negctl_${k}.txt)
    if [ "$npass" = 0 ] && [ "$nfail" -gt 0 ]; then echo "# verdict: control $k FAILS all $nfail cases with B >= 3 (B = 1, 2: the gradient is identically zero)" >> $sec
    else echo "!! control $k passes $npass cases with B >= 3: the gate does not catch it there" >> $sec; bad=1; fi
  done
  echo "# tools/negative_controls.sh supcon: $NEW against libmsig_hip_supcon1.so (make negctl SUPCON=1)" > "$OUT"
  for k in product 1; do [ -f $D/supcon_negctl_section_$k.log ] && cat $D/supcon_negctl_section_$k.log >> "$OUT"; done
  tail -n +1 "$OUT"
  exit $bad
fi
if [ "$1" = length ]; then
  OUT=${2:-length_negctl_out/length_negative_control.log}
  D=$(dirname "$OUT")
  shift; shift
  LIBS=${*:-product 1 2 3}
  OLDF='tests/test_parity_gpu.py tests/test_input_grad_gpu.py tests/test_channel_class_range_gpu.py tests/test_input_regimes_gpu.py'
  OLD='(test_parity_gpu and random_shapes and (137 or 250)) or test_input_grad_gpu or (test_channel_class_range_gpu and (137 or 250 or 511)) or (test_input_regimes_gpu and input_gradient)'
  NEW=tests/test_window_lengths_gpu.py
  mkdir -p "$D"
  bad=0
  for k in $LIBS; do
    if [ "$k" = product ]; then lib=$PWD/multimodalsignal_amd/libmsig_hip.so; else lib=$PWD/multimodalsignal_amd/csrc/build/libmsig_hip_length$k.so; fi
    sec=$D/length_negctl_section_$k.log
    [ -f "$lib" ] || { echo "## library: $(basename $lib): missing" > $sec; bad=1; continue; }
    MSIG_LIB=$lib timeout -k 10 420 python -m pytest $NEW -q -rA -p no:cacheprovider > $D/length_negctl_${k}_new.txt 2>&1; rc=$?
    echo "## library: $(basename $lib)" > $sec
    echo "# new file, $NEW (exit $rc):   $(tail -1 $D/length_negctl_${k}_new.txt)" >> $sec
    if [ "$k" = product ]; then grep -E "^(PASSED|FAILED) " $D/length_negctl_${k}_new.txt | sed 's/ - .*//' | sort >> $sec
    else grep -E "^FAILED " $D/length_negctl_${k}_new.txt | sed 's/ - .*//' | sort >> $sec; fi
    if [ $rc != 0 ] && [ $rc != 1 ]; then echo "!! abnormal exit $rc: stopped here" >> $sec; bad=2; break; fi
    nfail=$(grep -c "^FAILED " $D/length_negctl_${k}_new.txt)
    if [ "$k" = product ]; then
      [ $rc = 0 ] || { echo "!! the product library must pass the new file" >> $sec; bad=1; }
      continue
    fi
    if [ "$nfail" -gt 0 ]; then echo "# verdict: control $k FAILS $nfail new cases" >> $sec
    else echo "!! control $k fails no new case: the new file does not catch it" >> $sec; bad=1; fi
    MSIG_LIB=$lib timeout -k 10 900 python -m pytest $OLDF -q -rA -p no:cacheprovider -k "$OLD" > $D/length_negctl_${k}_old.txt 2>&1; rc=$?
    echo "# cases that ran unaligned lengths before, $OLDF -k \"$OLD\" (exit $rc):   $(tail -1 $D/length_negctl_${k}_old.txt)" >> $sec
    grep -E "^FAILED " $D/length_negctl_${k}_old.txt | sed 's/ - .*//' | sort >> $sec
    if [ $rc != 0 ] && [ $rc != 1 ]; then echo "!! abnormal exit $rc: stopped here" >> $sec; bad=2; break; fi
    if [ $rc = 0 ]; then echo "# verdict: the cases the suite had do NOT notice control $k" >> $sec
    else echo "!! the cases the suite had notice control $k: the slip is not confined to the new lengths" >> $sec; bad=1; fi
  done
  echo "# tools/negative_controls.sh length: $NEW and the unaligned cases the suite had against libmsig_hip_length<k>.so (make negctl LENGTH=k)" > "$OUT"
  for k in product 1 2 3; do [ -f $D/length_negctl_section_$k.log ] && cat $D/length_negctl_section_$k.log >> "$OUT"; done
  tail -n +1 "$OUT"
  exit $bad
fi
if [ "$1" = input ]; then
  OUT=${2:-input_negctl_out/input_negative_control.log}
  D=$(dirname "$OUT")
  shift; shift
  LIBS=${*:-product 1 2}
  OLD='golden_case or ws6'
  NEW='tests/test_input_regimes_gpu.py tests/test_adapt_gpu.py::test_both_stages_against_the_float64_restatement'
  want() { case $1 in 1) echo offset;; 2) echo units_small;; esac; }
  mkdir -p "$D"
  bad=0
  for k in $LIBS; do
    if [ "$k" = product ]; then lib=$PWD/multimodalsignal_amd/libmsig_hip.so; else lib=$PWD/multimodalsignal_amd/csrc/build/libmsig_hip_input$k.so; fi
    sec=$D/input_negctl_section_$k.log
    [ -f "$lib" ] || { echo "## library: $(basename $lib): missing" > $sec; bad=1; continue; }
    MSIG_LIB=$lib timeout -k 10 420 python -m pytest $NEW -q -rA -p no:cacheprovider > $D/input_negctl_${k}_new.txt 2>&1; rc=$?
    echo "## library: $(basename $lib)" > $sec
    echo "# new cases, $NEW (exit $rc):   $(tail -1 $D/input_negctl_${k}_new.txt)" >> $sec
    grep -E "^(PASSED|FAILED) " $D/input_negctl_${k}_new.txt | sed 's/ - .*//' | sort >> $sec
    if [ $rc != 0 ] && [ $rc != 1 ]; then echo "!! abnormal exit $rc: stopped here" >> $sec; bad=2; break; fi
    nfail=$(grep -c "^FAILED " $D/input_negctl_${k}_new.txt)
    if [ "$k" = product ]; then
      [ $rc = 0 ] || { echo "!! the product library must pass the new cases" >> $sec; bad=1; }
      continue
    fi
    nwant=$(grep "^FAILED " $D/input_negctl_${k}_new.txt | grep -c "$(want $k)")
    if [ "$nwant" -gt 0 ]; then echo "# verdict: control $k FAILS $nfail new cases, $nwant of them under $(want $k)" >> $sec
    else echo "!! control $k fails no new case under $(want $k) ($nfail failures in all): the new cases do not catch it" >> $sec; bad=1; fi
    MSIG_LIB=$lib timeout -k 10 600 python -m pytest tests/test_parity_gpu.py -q -rA -p no:cacheprovider -k "$OLD" > $D/input_negctl_${k}_old.txt 2>&1; rc=$?
    echo "# old selection, tests/test_parity_gpu.py -k \"$OLD\" (exit $rc):   $(tail -1 $D/input_negctl_${k}_old.txt)" >> $sec
    grep -E "^FAILED " $D/input_negctl_${k}_old.txt | sed 's/ - .*//' | sort >> $sec
    if [ $rc != 0 ] && [ $rc != 1 ]; then echo "!! abnormal exit $rc: stopped here" >> $sec; bad=2; break; fi
    if [ $rc = 0 ]; then echo "# verdict: the old selection does NOT notice control $k" >> $sec; else echo "# verdict: the old selection notices control $k" >> $sec; fi
    if [ "$k" = 1 ] && [ $rc != 0 ]; then echo "!! control 1 is the arithmetic the old selection always ran: it must pass it" >> $sec; bad=1; fi
  done
  echo "# tools/negative_controls.sh input: $NEW and tests/test_parity_gpu.py -k \"$OLD\" against libmsig_hip_input<k>.so (make negctl INPUT=k)" > "$OUT"
  for k in product 1 2; do [ -f $D/input_negctl_section_$k.log ] && cat $D/input_negctl_section_$k.log >> "$OUT"; done
  tail -n +1 "$OUT"
  exit $bad
fi
if [ "$1" = range ]; then
  OUT=${2:-range_negctl_out/range_negative_control.log}
  D=$(dirname "$OUT")
  shift; shift
  LIBS=${*:-product 1 2 3}
  OLD='golden_case or ws6'
  NEW=tests/test_channel_class_range_gpu.py
  mkdir -p "$D"
  bad=0
  for k in $LIBS; do
    if [ "$k" = product ]; then lib=$PWD/multimodalsignal_amd/libmsig_hip.so; else lib=$PWD/multimodalsignal_amd/csrc/build/libmsig_hip_range$k.so; fi
    sec=$D/range_negctl_section_$k.log
    [ -f "$lib" ] || { echo "## library: $(basename $lib): missing" > $sec; bad=1; continue; }
    MSIG_LIB=$lib timeout -k 10 420 python -m pytest $NEW -q -rA -p no:cacheprovider > $D/range_negctl_${k}_new.txt 2>&1; rc=$?
    echo "## library: $(basename $lib)" > $sec
    echo "# new file, $NEW (exit $rc):   $(tail -1 $D/range_negctl_${k}_new.txt)" >> $sec
    grep -E "^(PASSED|FAILED) " $D/range_negctl_${k}_new.txt | sed 's/ - .*//' | sort >> $sec
    if [ $rc != 0 ] && [ $rc != 1 ]; then echo "!! abnormal exit $rc: stopped here" >> $sec; bad=2; break; fi
    nfail=$(grep -c "^FAILED " $D/range_negctl_${k}_new.txt)
    if [ "$k" = product ]; then
      [ $rc = 0 ] || { echo "!! the product library must pass the new file" >> $sec; bad=1; }
      continue
    fi
    if [ "$nfail" -gt 0 ]; then echo "# verdict: control $k FAILS $nfail new cases" >> $sec
    else echo "!! control $k fails no new case: the new file does not catch it" >> $sec; bad=1; fi
    MSIG_LIB=$lib timeout -k 10 600 python -m pytest tests/test_parity_gpu.py -q -rA -p no:cacheprovider -k "$OLD" > $D/range_negctl_${k}_old.txt 2>&1; rc=$?
    echo "# old selection, tests/test_parity_gpu.py -k \"$OLD\" (exit $rc):   $(tail -1 $D/range_negctl_${k}_old.txt)" >> $sec
    grep -E "^FAILED " $D/range_negctl_${k}_old.txt | sed 's/ - .*//' | sort >> $sec
    if [ $rc != 0 ] && [ $rc != 1 ]; then echo "!! abnormal exit $rc: stopped here" >> $sec; bad=2; break; fi
    if [ $rc = 0 ]; then echo "# verdict: the old selection does NOT notice control $k" >> $sec; else echo "# verdict: the old selection notices control $k" >> $sec; fi
  done
  echo "# tools/negative_controls.sh range: $NEW and tests/test_parity_gpu.py -k \"$OLD\" against libmsig_hip_range<k>.so (make negctl RANGE=k)" > "$OUT"
  for k in product 1 2 3; do [ -f $D/range_negctl_section_$k.log ] && cat $D/range_negctl_section_$k.log >> "$OUT"; done
  tail -n +1 "$OUT"
  exit $bad
fi
if [ "$1" = regime ]; then
  OUT=${2:-regime_negctl_out/regime_negative_control.log}
  D=$(dirname "$OUT")
  shift; shift
  LIBS=${*:-product 1 2 3 4}
  OLD='golden_case or ws6'
  want() { case $1 in 1|2) echo z_sat;; 3) echo bn_affine;; 4) echo head_sat;; esac; }
  mkdir -p "$D"
  bad=0
  for k in $LIBS; do
    if [ "$k" = product ]; then lib=$PWD/multimodalsignal_amd/libmsig_hip.so; else lib=$PWD/multimodalsignal_amd/csrc/build/libmsig_hip_regime$k.so; fi
    sec=$D/regime_negctl_section_$k.log
    [ -f "$lib" ] || { echo "## library: $(basename $lib): missing" > $sec; bad=1; continue; }
    MSIG_LIB=$lib timeout -k 10 420 python -m pytest tests/test_trained_regimes_gpu.py -q -rA -p no:cacheprovider > $D/regime_negctl_${k}_new.txt 2>&1; rc=$?
    echo "## library: $(basename $lib)" > $sec
    echo "# new file, tests/test_trained_regimes_gpu.py (exit $rc):   $(tail -1 $D/regime_negctl_${k}_new.txt)" >> $sec
    grep -E "^(PASSED|FAILED) " $D/regime_negctl_${k}_new.txt | sed 's/ - .*//' | sort >> $sec
    if [ $rc != 0 ] && [ $rc != 1 ]; then echo "!! abnormal exit $rc: stopped here" >> $sec; bad=2; break; fi
    nfail=$(grep -c "^FAILED " $D/regime_negctl_${k}_new.txt)
    if [ "$k" = product ]; then
      [ $rc = 0 ] || { echo "!! the product library must pass the new file" >> $sec; bad=1; }
      continue
    fi
    nwant=$(grep "^FAILED " $D/regime_negctl_${k}_new.txt | grep -c "$(want $k)")
    if [ "$nwant" -gt 0 ]; then echo "# verdict: control $k FAILS $nfail new cases, $nwant of them under $(want $k)" >> $sec
    else echo "!! control $k fails no new case under $(want $k) ($nfail failures in all): the new file does not catch it" >> $sec; bad=1; fi
    MSIG_LIB=$lib timeout -k 10 600 python -m pytest tests/test_parity_gpu.py -q -rA -p no:cacheprovider -k "$OLD" > $D/regime_negctl_${k}_old.txt 2>&1; rc=$?
    echo "# old selection, tests/test_parity_gpu.py -k \"$OLD\" (exit $rc):   $(tail -1 $D/regime_negctl_${k}_old.txt)" >> $sec
    grep -E "^FAILED " $D/regime_negctl_${k}_old.txt | sed 's/ - .*//' | sort >> $sec
    if [ $rc != 0 ] && [ $rc != 1 ]; then echo "!! abnormal exit $rc: stopped here" >> $sec; bad=2; break; fi
    if [ $rc = 0 ]; then echo "# verdict: the old selection does NOT notice control $k" >> $sec; else echo "# verdict: the old selection notices control $k" >> $sec; fi
  done
  echo "# tools/negative_controls.sh regime: tests/test_trained_regimes_gpu.py and tests/test_parity_gpu.py -k \"$OLD\" against libmsig_hip_regime<k>.so (make negctl REGIME=k)" > "$OUT"
  for k in product 1 2 3 4; do [ -f $D/regime_negctl_section_$k.log ] && cat $D/regime_negctl_section_$k.log >> "$OUT"; done
  tail -n +1 "$OUT"
  exit $bad
fi
SEL='golden_case_stages or (random_shapes and (ws6 or split) and (40-6-2-512 or 33-3-3-256 or 3100-6-2-64 or 17-6-2-320))'
OUT=${1:-gpurun_out/r05_negative_control.log}
mkdir -p gpurun_out
: > "$OUT"
echo "# tools/negative_controls.sh: python -m pytest tests/test_parity_gpu.py -k \"$SEL\"  (4 golden cases + 4 shapes x the two shipped form sets = 12 cases)" >> "$OUT"
bad=0
for k in product 1 2 3 4 5 9; do
  if [ "$k" = product ]; then lib=$PWD/multimodalsignal_amd/libmsig_hip.so; else lib=$PWD/multimodalsignal_amd/csrc/build/libmsig_hip_negctl$k.so; fi
  [ -f "$lib" ] || { echo "missing $lib" >> "$OUT"; bad=1; continue; }
  MSIG_LIB=$lib timeout -k 10 400 python -m pytest tests/test_parity_gpu.py -q -rA -p no:cacheprovider -k "$SEL" > gpurun_out/negctl_$k.txt 2>&1
  echo "## library: $(basename $lib)   ->   $(tail -1 gpurun_out/negctl_$k.txt)" >> "$OUT"
  grep -E "^(PASSED|FAILED) " gpurun_out/negctl_$k.txt | sed 's/ - .*//' | sort >> "$OUT"
  npass=$(grep -c "^PASSED " gpurun_out/negctl_$k.txt); nfail=$(grep -c "^FAILED " gpurun_out/negctl_$k.txt)
  if [ "$k" = product ]; then [ "$nfail" = 0 ] && [ "$npass" = 12 ] || { echo "!! the product library must pass all 12 cases" >> "$OUT"; bad=1; }
  else [ "$npass" = 0 ] && [ "$nfail" = 12 ] || { echo "!! control $k passed $npass of 12 cases: the gate does not catch it there" >> "$OUT"; bad=1; }; fi
done
tail -n +1 "$OUT"
exit $bad
