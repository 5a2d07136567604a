// track_scene.h -- the track scene rpe_triangulate_tracks and rpe_bundle_windows share (include/rpe_amd.h): tracks in CSR form,
// one world-to-camera pose per frame, one K or one camera per frame.  The caller's view of it and its argument check.  Plain
// C++, nothing of HIP: pointers in, nullptr or the refusal text out, so tests/native/track_scene_host.cpp runs it on the host.
#pragma once
#include "../../include/rpe_amd.h"

#define RPE_NULL_ARGUMENT_TEXT "a null argument or a count out of range"   // the refusal that names no argument (rpe_invalid's default)

struct RpeSceneArgs {
    int n_tracks;
    const int32_t *track_start, *obs_frame;   // [n_tracks + 1], [n_obs]; n_obs = track_start[n_tracks]
    const float *obs_xy;                      // [n_obs][2]
    int n_frames;
    const double *R_abs, *T_abs, *K;          // [n_frames][9], [n_frames][3]; [9] or, with K null,
    const rpe_camera *cams;                   // [n_frames]
};

// Phase 1, in front of the empty-call return: the scalars and the CSR shape of track_start (when given; n_tracks + 1 entries
// are read, behind the test of n_tracks).  The cameras are the caller's to check (check_cameras, rpe_host.h).
static inline const char *rpe_scene_check_shape(const RpeSceneArgs &a)
{
    if (a.n_tracks < 0) return "n_tracks must be >= 0";
    if (a.n_frames < 1) return "n_frames must be >= 1";
    if ((a.K == nullptr) == (a.cams == nullptr)) return "exactly one of K and cams must be given";
    if (a.track_start) {
        if (a.track_start[0] != 0) return "track_start[0] must be 0";
        for (int k = 0; k < a.n_tracks; ++k)
            if (a.track_start[k + 1] < a.track_start[k]) return "track_start must not decrease";
    }
    return nullptr;
}

// Phase 2, behind it and behind phase 1: the pointers that are read, then the range of obs_frame.  *n_obs: the observations
// (0 without tracks, track_start is then not needed)
static inline const char *rpe_scene_check_arrays(const RpeSceneArgs &a, size_t *n_obs)
{
    *n_obs = 0;
    if (!a.R_abs || !a.T_abs || (a.n_tracks > 0 && !a.track_start)) return RPE_NULL_ARGUMENT_TEXT;
    const size_t no = a.n_tracks > 0 ? (size_t)a.track_start[a.n_tracks] : 0;
    if (no > 0 && (!a.obs_frame || !a.obs_xy)) return RPE_NULL_ARGUMENT_TEXT;
    for (size_t o = 0; o < no; ++o)
        if (a.obs_frame[o] < 0 || a.obs_frame[o] >= a.n_frames) return "a frame index outside 0 ... n_frames - 1";
    *n_obs = no;
    return nullptr;
}
