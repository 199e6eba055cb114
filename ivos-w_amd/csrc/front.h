// Internal launchers shared between assess_front.hip and assess.hip.
#pragma once
#include "common.h"

namespace ivosw {
struct RoiNorm {
    float mean[3];
    float std[3];
    const float* dev;  // optional device copy {mean[3], std[3]} (the Encoder.mean/std buffers of a checkpoint)
};
// Which frame and which mask plane sample b of a batch reads.  Samples are object-major: b = obj * n_frames + frame, so
// O objects of one n-frame video share ONE copy of the frames (utils/utils_agent.py:118-119 scores one object at a time on
// the same all_F): frame = tf + (b % n_frames) * 3*H*W, mask = tp + (b / n_frames) * stride_obj + (b % n_frames) * stride_frame
// (strides in elements).  A plain batch is {n_frames = B, stride_frame = H*W, stride_obj = 0}.
struct SampleMap {
    int n_frames;
    long stride_frame, stride_obj;
};
// Where the sampler reads its colours: fp32 planes [n,3,H,W] in 0..1 (u8 = 0), or RGBX8 bytes [n,H,W,4] (u8 = 1, 4-byte aligned:
// include/ivosw.h).  It travels with the frames through the chunk loop, the two-stream split and the SampleMap indirection.
struct FrameSrc {
    const void* p;
    int u8;
};
// Several videos in one launch.  Units are numbered video-major, then object-major inside a video: u = first[v] + obj * n_frames[v] +
// frame.  The table travels BY VALUE in the kernel arguments (under 2 KB for IVOSW_MAX_VIDEOS = 32): no allocation and no copy, so the
// multi-video entries stay capture-safe.  A workgroup finds the video of its unit with a branch-free count over first[] (entries behind
// the last video hold INT_MAX) - scalar loads and compares, uniform per workgroup - and reads that video's row through scalar loads.
struct VideoDesc {
    const void* frames;                  // fp32 [n,3,H,W] or RGBX8 [n,H,W,4] (u8)
    const float* masks;
    long stride_frame, stride_obj;       // of the mask planes, in elements
    int n_frames, n_obj, H, W;
    int u8;                              // frame source: 0 fp32 planes, 1 RGBX8
    int vec_ok;                          // the scan may use 16-byte loads on this video's planes (what launch_mask_bbox derives)
    // Label-map masks (include/ivosw.h: ivosw_labels_t).  lab != NULL: the video's masks are ONE uint8 [n_frames,H,W] map, object obj
    // owns the value obj + 1, and the plane of unit (frame, obj) is (lab[frame * lab_stride + i] == obj + 1) ? 1.0f : 0.0f - `masks` and
    // its strides are not looked at.  vec_ok then says: H * W % 16 == 0, map base and lab_stride 16-byte aligned (16 pixels per load).
    const uint8_t* lab;
    long lab_stride;                     // between frames, in elements (= bytes)
};
struct VideoTable {
    VideoDesc v[IVOSW_MAX_VIDEOS];
    int first[IVOSW_MAX_VIDEOS];         // first unit of video i; INT_MAX for i >= n
    int n, units;
    int any_lab;                         // host only: some video is a label video - the launchers then run the Lab instantiations
};
// The table and the per-call pointer arrays next to it are kernel ARGUMENTS: together they must stay inside the 4 KB a launch carries.
static_assert(sizeof(VideoTable) + IVOSW_MAX_VIDEOS * 16 + 64 <= 4096, "VideoTable + DeltaArgs no longer fit the kernel arguments");
// Validates the caller's array (every refusal of include/ivosw.h, the message names the video) and fills the table.
// labels (may be NULL): the HOST array of the *_lab entries; labels[v].map != NULL makes video v a label video.
int video_table_build(const ivosw_video_t* videos, int n_videos, const char* who, VideoTable* out, const ivosw_labels_t* labels = nullptr);
// ids != NULL: rows [b0, b0 + B) of a unit list (a device array) instead of the units [b0, b0 + B): row b works on unit ids[b0 + b]
void launch_mask_bbox_multi(const VideoTable& vt, int b0, int B, float* yxhw, int32_t* scratch, hipStream_t st, const int32_t* ids = nullptr);
void launch_roi_sample_multi(const VideoTable& vt, const float* yxhw, int b0, int B, int dtype, const RoiNorm& nrm, void* roi, hipStream_t st,
                             const int32_t* ids = nullptr);
// scores[ids[i]] = compact[i], i < n (ids outside [0, units) are dropped)
void launch_scatter_units(const float* compact, const int32_t* ids, int n, int units, float* scores, hipStream_t st);
void launch_mask_bbox(const float* tp, int b0, int B, int H, int W, const SampleMap& sm, float* yxhw, int32_t* scratch, hipStream_t st);
void launch_roi_sample(const FrameSrc& fs, const float* tp, const float* yxhw, int b0, int B, int H, int W, int dtype,
                       const SampleMap& sm, const RoiNorm& nrm, void* roi, hipStream_t st);
}  // namespace ivosw
