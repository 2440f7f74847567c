#!/bin/bash
# PSNR / SSIM of a run's per-segment dumps on the MI355X: counterpart of the reference's calculate_metrics.sh (same variables).
# Compares $VIDEO_PATH/<episode>/predictions_gt_$SEGMENT_ID with predictions_$SEGMENT_ID and writes $VIDEO_PATH/$RESULT_PATH.
# FVD, LPIPS and the latent MSEs need network weights this project does not ship; the JSON lists what was not computed under
# "not_computed".
# LPIPS_WEIGHTS (optional: one file with a lpips.LPIPS state dict, or torchvision's AlexNet and the lpips package's alex.pth, as
# .safetensors or torch checkpoints) adds LPIPS; LPIPS_CHANNEL_ORDER (default bgr, as the reference feeds its network; rgb) goes with it.
# FVD_WEIGHTS (optional: a state dict in InceptionI3d's key layout, e.g. i3d_pretrained_400.pt, as .safetensors or a torch checkpoint) adds
# FVD, the styleganv method at every clip length from 10 frames; FVD_CHANNEL_ORDER (default bgr, as the reference feeds its network; rgb).
# LATENT_MSE_WEIGHTS (optional: a state dict in timm inception_v4's key layout, as .safetensors or a torch checkpoint) adds latent_mse
# and loop_closure_latent_mse (the last frame alone); LATENT_MSE_CHANNEL_ORDER (default bgr, as the reference feeds its network; rgb).
# WS_METRICS=1 adds the latitude-weighted forms for equirectangular frames (a row counts with the cosine of its latitude; not in the
# reference): ws_psnr and ws_ssim, and ws_lpips when LPIPS_WEIGHTS is set.
# PROJECTION=cube scores every clip on its six 90-degree perspective viewports (front, right, back, left, up, down: each episode and face
# one video of every selected metric) instead of the flat panorama; VIEWPORT_SIZE (default: frame width / 4) is a viewport's side.  It
# cannot be combined with WS_METRICS: latitude weights mean nothing on a perspective face.
# PAIR_BY_NAME (default: true for SEGMENT_ID > 0) pairs the frame files both folders share: a later segment holds 24 generated and
# 25 ground-truth frames, on which the reference's shape assertion fails.
set -e
cd "$(dirname "$0")"

CKPT=${CKPT:-MODELS/evoworld_curve_unity}
OUTPUT_ROOT=${OUTPUT_ROOT:-output}
VIDEO_PATH=${VIDEO_PATH:-$OUTPUT_ROOT/$(basename $CKPT)/eval_unity_curve}
NUM_VIDEO=${NUM_VIDEO:-200}
RESULT_PATH=${RESULT_PATH:-eval_score.json}
SEGMENT_ID=${SEGMENT_ID:-2}  # Change this to evaluate different segments (0, 1, 2)
if [ -z "$PAIR_BY_NAME" ]; then
  if [ "$SEGMENT_ID" -gt 0 ]; then PAIR_BY_NAME=true; else PAIR_BY_NAME=false; fi
fi

make -s -C evoworld_amd/csrc

CMD="-m evoworld_amd.metrics --data_path $VIDEO_PATH --gt_subdir predictions_gt_$SEGMENT_ID --gen_subdir predictions_$SEGMENT_ID \
 --result_file $RESULT_PATH --test_length 25 --num_video $NUM_VIDEO"
[ "$PAIR_BY_NAME" = true ] && CMD="$CMD --pair_by_name"
METRICS=psnr,ssim
[ -n "$LPIPS_WEIGHTS" ] && METRICS=psnr,ssim,lpips && CMD="$CMD --lpips_weights $LPIPS_WEIGHTS --lpips_channel_order ${LPIPS_CHANNEL_ORDER:-bgr}"
[ -n "$FVD_WEIGHTS" ] && METRICS=$METRICS,fvd && CMD="$CMD --fvd_weights $FVD_WEIGHTS --fvd_channel_order ${FVD_CHANNEL_ORDER:-bgr}"
[ -n "$LATENT_MSE_WEIGHTS" ] && METRICS=$METRICS,latent_mse,loop_closure_latent_mse \
  && CMD="$CMD --latent_mse_weights $LATENT_MSE_WEIGHTS --latent_mse_channel_order ${LATENT_MSE_CHANNEL_ORDER:-bgr}"
if [ "${WS_METRICS:-0}" = 1 ]; then
  METRICS=$METRICS,ws_psnr,ws_ssim
  [ -n "$LPIPS_WEIGHTS" ] && METRICS=$METRICS,ws_lpips
fi
[ -n "$PROJECTION" ] && CMD="$CMD --projection $PROJECTION"
[ -n "$VIEWPORT_SIZE" ] && CMD="$CMD --viewport_size $VIEWPORT_SIZE"
CMD="$CMD --metrics $METRICS"
python $CMD
