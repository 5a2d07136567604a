// Stand-alone check of csrc/track_scene.h (the argument check rpe_triangulate_tracks and rpe_bundle_windows share), built by
// tests/test_track_scene_cpu.py with the address and undefined-behaviour sanitizers.  Every array is a heap block of exactly
// its length, so a read in front of the check of its pointer or length is a sanitizer error.  The two phases run as the entry
// points run them: phase 2 only behind a phase 1 that passed.
#include <cstdio>
#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "track_scene.h"

struct Scene {
    std::unique_ptr<int32_t[]> ts, of;
    std::unique_ptr<float[]> xy;
    std::unique_ptr<double[]> R, T, K;
    std::unique_ptr<rpe_camera[]> cams;
    RpeSceneArgs a;
    // starts[] = track_start (n_tracks + 1 entries), frames[] = obs_frame (as many as starts ends at); one K
    Scene(std::vector<int32_t> starts, std::vector<int32_t> frames, int n_frames)
    {
        const size_t no = frames.size(), nf = (size_t)(n_frames > 0 ? n_frames : 0);
        ts.reset(new int32_t[starts.size()]); of.reset(new int32_t[no]); xy.reset(new float[2 * no]());
        R.reset(new double[9 * nf]()); T.reset(new double[3 * nf]()); K.reset(new double[9]()); cams.reset(new rpe_camera[nf]());
        std::copy(starts.begin(), starts.end(), ts.get());
        std::copy(frames.begin(), frames.end(), of.get());
        a = {(int)starts.size() - 1, ts.get(), of.get(), xy.get(), n_frames, R.get(), T.get(), K.get(), nullptr};
    }
};

static const char *check(const RpeSceneArgs &a, size_t *n_obs)
{
    if (const char *what = rpe_scene_check_shape(a)) return what;
    return rpe_scene_check_arrays(a, n_obs);
}

static long accepted = 0, refused = 0, bad = 0;
static void accept(const RpeSceneArgs &a, size_t want_obs)
{
    size_t no = ~(size_t)0;
    const char *what = check(a, &no);
    if (what || no != want_obs) { ++bad; std::printf("refused a valid scene: %s (%zu observations)\n", what ? what : "-", no); }
    ++accepted;
}
static void refuse(const RpeSceneArgs &a, const char *want)
{
    size_t no;
    const char *what = check(a, &no);
    if (!what || std::strcmp(what, want) != 0) { ++bad; std::printf("wanted '%s', got '%s'\n", want, what ? what : "accepted"); }
    ++refused;
}

int main()
{
    const std::vector<int32_t> starts = {0, 2, 4, 7}, frames = {0, 1, 1, 2, 0, 1, 2};
    // valid: no track, a track without observations, 3 tracks / 7 observations / 3 frames; each with K and with cameras
    for (int with_cams = 0; with_cams < 2; ++with_cams) {
        Scene none({0}, {}, 1), empty({0, 0}, {}, 2), three(starts, frames, 3);
        struct { Scene *s; size_t n_obs; } valid[3] = {{&none, 0}, {&empty, 0}, {&three, 7}};
        for (auto &v : valid) {
            if (with_cams) { v.s->a.K = nullptr; v.s->a.cams = v.s->cams.get(); }
            accept(v.s->a, v.n_obs);
        }
        // no track needs no track_start, and no observation no observation arrays
        none.a.track_start = nullptr; accept(none.a, 0);
        empty.a.obs_frame = nullptr; empty.a.obs_xy = nullptr; accept(empty.a, 0);
    }
    // every single fault, on the three-track scene
    const char *null_text = RPE_NULL_ARGUMENT_TEXT, *range_text = "a frame index outside 0 ... n_frames - 1";
    { Scene s(starts, frames, 3); s.a.n_tracks = -1; refuse(s.a, "n_tracks must be >= 0"); }
    { Scene s(starts, frames, 0); refuse(s.a, "n_frames must be >= 1"); }
    { Scene s(starts, frames, 3); s.a.cams = s.cams.get(); refuse(s.a, "exactly one of K and cams must be given"); }
    { Scene s(starts, frames, 3); s.a.K = nullptr; refuse(s.a, "exactly one of K and cams must be given"); }
    { Scene s({1, 2, 4, 7}, frames, 3); refuse(s.a, "track_start[0] must be 0"); }
    // decreasing, with an entry past the observations in front of the fault and at the end: neither is used as a length
    { Scene s({0, 9, 4, 7}, frames, 3); refuse(s.a, "track_start must not decrease"); }
    { Scene s({0, 2, 1, 9}, frames, 3); refuse(s.a, "track_start must not decrease"); }
    { Scene s(starts, frames, 3); s.a.track_start = nullptr; refuse(s.a, null_text); }
    { Scene s(starts, frames, 3); s.a.R_abs = nullptr; refuse(s.a, null_text); }
    { Scene s(starts, frames, 3); s.a.T_abs = nullptr; refuse(s.a, null_text); }
    { Scene s(starts, frames, 3); s.a.obs_frame = nullptr; refuse(s.a, null_text); }
    { Scene s(starts, frames, 3); s.a.obs_xy = nullptr; refuse(s.a, null_text); }
    { Scene s(starts, {0, 1, 1, 2, 0, 1, 3}, 3); refuse(s.a, range_text); }
    { Scene s(starts, {-1, 1, 1, 2, 0, 1, 2}, 3); refuse(s.a, range_text); }
    std::printf("%ld accepted, %ld refused, %ld bad\n", accepted, refused, bad);
    return bad != 0;
}
