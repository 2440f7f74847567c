#!/bin/bash
# N-segment loop-consistency run (generation -> reprojection -> 3D memory -> next segment) on the MI355X-native hot path: counterpart of the reference's run_unified_pipeline.sh
# (same variables, same flags).  With no checkpoint under $CKPT the U-Net is randomly initialised (RANDOM_INIT=true) and the
# VAE / CLIP / VGGT stages are the synthetic stand-ins of evoworld_amd.stages (override with STAGES=pkg.mod:factory).
set -e
cd "$(dirname "$0")"
export HSA_ENABLE_IPC_MODE_LEGACY=0

CKPT=${CKPT:-MODELS/evoworld_curve_unity}
BASE_FOLDER=${BASE_FOLDER:-example/case_000}
OUTPUT_ROOT=${OUTPUT_ROOT:-output}
SAVE_DIR=$OUTPUT_ROOT/$(basename $CKPT)/unified_demo
START_IDX=${START_IDX:-0}
NUM_DATA_PER_GPU=${NUM_DATA_PER_GPU:-1}
NUM_SEGMENTS=${NUM_SEGMENTS:-3}
CURVE_PATH=${CURVE_PATH:-true}
NUM_GPUS=${NUM_GPUS:-1}
STEPS=${STEPS:-25}

[ -d "$CKPT" ] || RANDOM_INIT=true
make -s -C evoworld_amd/csrc

CMD="unified_loop_consistency.py --unet_path $CKPT --svd_path $CKPT --base_folder $BASE_FOLDER --save_dir $SAVE_DIR \
 --num_data $((NUM_DATA_PER_GPU * NUM_GPUS)) --start_idx $START_IDX --num_segments $NUM_SEGMENTS --num_frames 25 \
 --num_inference_steps $STEPS --save_frames"
[ "$CURVE_PATH" = true ] && CMD="$CMD --curve_path"
[ "$RANDOM_INIT" = true ] && CMD="$CMD --random_init"
[ -n "$STAGES" ] && CMD="$CMD --stages $STAGES"
[ "$QKV_FP8" = 1 ] && CMD="$CMD --qkv_fp8"      # opt-in fp8 (e4m3) q / k / v projections: BASELINE.json configs[4]
[ "$EXPORT_GLB" = 1 ] && CMD="$CMD --export_glb"   # opt-in: glbscene_{seg}.glb of every hand-off's 3D memory
[ -n "$MEMORY_VOXEL_SIZE" ] && CMD="$CMD --memory_voxel_size $MEMORY_VOXEL_SIZE"   # opt-in voxel-grid downsample of the memory
[ "$SAVE_VIDEO" = 1 ] && CMD="$CMD --save_video"   # opt-in: navigated.avi (+ original.avi) per episode, Motion-JPEG encoded on the device
[ "$DEVICE_PNG" = 1 ] && CMD="$CMD --device_png"   # opt-in: the --save_frames PNG files are encoded on the device (same pixels)
[ -n "$DEPTH_STAGE" ] && CMD="$CMD --depth_stage $DEPTH_STAGE"   # opt-in: mvs = plane-sweep stereo depth from the generated frames (default: synthetic)
[ -n "$MVS_PLANES" ] && CMD="$CMD --mvs_planes $MVS_PLANES"
[ -n "$MVS_SOURCES" ] && CMD="$CMD --mvs_sources $MVS_SOURCES"
[ -n "$MVS_AGGREGATE" ] && CMD="$CMD --mvs_aggregate $MVS_AGGREGATE"   # opt-in: sgm = semi-global aggregation of the sweep's cost volume (default: box)
[ -n "$MVS_P1" ] && CMD="$CMD --mvs_p1 $MVS_P1"
[ -n "$MVS_P2" ] && CMD="$CMD --mvs_p2 $MVS_P2"
[ -n "$MVS_PATHS" ] && CMD="$CMD --mvs_paths $MVS_PATHS"
[ -n "$MVS_COST" ] && CMD="$CMD --mvs_cost $MVS_COST"   # opt-in: zncc = match by normalised cross-correlation, for frames whose exposure or tone drifts (default: sad)
[ -n "$VIDEO_FPS" ] && CMD="$CMD --video_fps $VIDEO_FPS"
[ -n "$VIDEO_QUALITY" ] && CMD="$CMD --video_quality $VIDEO_QUALITY"

if [ "$NUM_GPUS" -gt 1 ]; then
  python -m torch.distributed.run --nnodes=1 --nproc-per-node "$NUM_GPUS" --master-addr 127.0.0.1 --master-port ${MASTER_PORT:-29511} $CMD
else
  python $CMD
fi
echo "Unified pipeline completed: $SAVE_DIR"
