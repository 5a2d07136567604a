"""Which calls behind the last run a handle serves, state by state.  One ORB / Hamming handle is brought into each state
in turn; in each, the eight calls that read the last run (the table at last_run_gate in csrc/rpe_api.hip) are made with
a valid count.  EXPECTED holds the outcome of every (state, call): served, or refused with a text.  It was taken from
the library before the gate was one function and is what that function has to reproduce.  A refusal changes nothing:
after all of a state's refusals, every call the state serves returns the bits it returned before.

The chunked state (a 512-pair host batch) stays with test_gpu_structure / test_gpu_refine / test_gpu_parity.

Scene and handle of test_gpu_call_sequences.py: synthetic.make_batch(4, K, cfg=9), frames interleaved, 640 x 480,
max_batch 8, nfeatures 1000."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LIST = [(0, 1), (2, 3), (4, 5), (6, 7), (1, 0), (5, 4)]
N = 2                                                      # pairs asked for: every run below has at least two
# the calls, by the names used below, and the entry point a refusal names
ENTRY = {"overflow": "rpe_fetch_overflow", "matched_points": "rpe_fetch_matched_points", "match_indices": "rpe_fetch_match_indices",
         "structure": "rpe_fetch_structure", "refine": "rpe_refine_poses", "scale_links": "rpe_scale_links",
         "guided": "rpe_guided_matches", "homographies": "rpe_pair_homographies"}
CALLS = list(ENTRY)

OK = None                                                  # served
NONE = "no batch or stream since the last stage-API call"
MORE = "more pairs than the last batch"
RESIZED = "the frame store was resized since the pair list"
NO_FRAME = "share no frame"
# state -> outcome per call, in the order of CALLS
EXPECTED = {
    "fresh":                    [MORE, OK, OK, NONE, NONE, NONE, NONE, NONE],
    "device batch":             [OK, OK, OK, OK, OK, NO_FRAME, OK, OK],
    "stream":                   [OK, OK, OK, OK, OK, OK, OK, OK],
    "K list":                   [OK, OK, OK, OK, OK, OK, OK, OK],
    "camera list":              [OK, OK, OK, OK, OK, OK, OK, OK],
    "K list, reserve":          [RESIZED, OK, OK, OK, OK, RESIZED, RESIZED, RESIZED],
    "camera list, reserve":     [RESIZED, OK, OK, NONE, NONE, NONE, NONE, NONE],
    "K list, set_cameras":      [OK, OK, OK, OK, OK, OK, OK, OK],
    "camera list, set_cameras": [OK, OK, OK, NONE, NONE, NONE, NONE, NONE],
    "list, put":                [MORE, OK, OK, NONE, NONE, NONE, NONE, NONE],
    "stage call":               [OK, OK, OK, NONE, NONE, NONE, NONE, NONE],
}


@pytest.fixture(scope="module")
def capi():
    from relative_pose_estimation_amd import _capi
    assert _capi.load().rpe_device_count() > 0, "no HIP device visible"
    return _capi


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint64) if x.dtype == np.float64 else x


def _round(capi, e, link):
    """the eight calls once: name -> the arrays returned, or the text of the refusal"""
    calls = {"overflow": lambda: (e.fetch_overflow(N),), "matched_points": lambda: e.fetch_matched_points(N),
             "match_indices": lambda: e.fetch_match_indices(N), "structure": lambda: e.fetch_structure(N),
             "refine": lambda: e.refine_poses(N), "scale_links": lambda: e.scale_links(*link),
             "guided": lambda: e.guided_matches(N), "homographies": lambda: e.pair_homographies(N)}
    out = {}
    for name in CALLS:
        try:
            out[name] = calls[name]()
        except capi.RpeError as err:
            out[name] = str(err)
    return out


@pytest.fixture(scope="module")
def walk(capi, K_vga):
    """state -> (the eight calls, the eight calls again), on one handle"""
    from relative_pose_estimation_amd import synthetic
    K = K_vga
    i1, i2, _, _ = synthetic.make_batch(4, K, cfg=9)
    frames = np.empty((8, 480, 640), np.uint8)
    frames[0::2] = i1; frames[1::2] = i2
    pairs = np.asarray(LIST)
    stream_link, list_link = ([0], [1], [1]), ([0], [4], [2])     # pairs (f0, f1), (f1, f2) / list entries (0, 1), (1, 0)
    e = capi.Engine(640, 480, max_batch=8, nfeatures=1000, max_matches=500)
    d1, d2, df = e.upload(i1[:2]), e.upload(i2[:2]), e.upload(frames)
    got = {}

    def klist():
        e.estimate_pairs(pairs[:, 0], pairs[:, 1], K)

    def camlist():
        e.estimate_pairs_cameras(pairs[:, 0], pairs[:, 1])

    def cameras():
        e.frames_set_cameras(np.arange(8), capi.Camera(K))

    def state(name, link):
        got[name] = (_round(capi, e, link), _round(capi, e, link))

    try:
        state("fresh", stream_link)
        R, t, inl, nm, st = e.estimate_batch_device(d1, d2, 2, K)
        assert not st.any() and (nm >= 100).all(), (st, nm)
        state("device batch", stream_link)
        p1, p2 = e.fetch_matched_points(2)
        points = ([p1[i, :nm[i]] for i in range(2)], [p2[i, :nm[i]] for i in range(2)])
        e.enqueue_stream_device(df, 8, K)
        e.fetch_results(7)
        state("stream", stream_link)
        e.frames_reserve(8)
        e.frames_put(frames, np.arange(8))
        klist()
        state("K list", list_link)
        cameras()
        camlist()
        state("camera list", list_link)
        klist()
        e.frames_reserve(12)
        state("K list, reserve", list_link)
        camlist()
        e.frames_reserve(8)
        state("camera list, reserve", list_link)
        klist()
        cameras()
        state("K list, set_cameras", list_link)
        camlist()
        cameras()
        state("camera list, set_cameras", list_link)
        klist()
        e.frames_put(frames[:2], [0, 1])
        state("list, put", list_link)
        e.estimate_batch_device(d1, d2, 2, K)
        e.find_essential(*points, K)
        state("stage call", stream_link)
        # a refused call leaves its own text: the stage call's refusal is not what a later, silent refusal reports
        with pytest.raises(capi.RpeError) as first:
            e.fetch_structure(N)
        with pytest.raises(capi.RpeError) as second:
            e.fetch_results(0)
        got["texts"] = (str(first.value), str(second.value))
    finally:
        e.synchronize()
        for d in (d1, d2, df):
            e.device_free(d)
        e.close()
    return got


@pytest.mark.parametrize("state", list(EXPECTED))
def test_state_serves_and_refuses_as_recorded(walk, state):
    first, again = walk[state]
    for name, want in zip(CALLS, EXPECTED[state]):
        for got in (first[name], again[name]):
            print(state, "|", name, "|", got if isinstance(got, str) else "served")
            if want is OK:
                assert not isinstance(got, str), (state, name, got)
            else:
                assert isinstance(got, str) and f"{ENTRY[name]}: " in got and want in got, (state, name, got)


@pytest.mark.parametrize("state", list(EXPECTED))
def test_refusals_leave_the_state_alone(walk, state):
    """the second round ran behind every refusal of the first: what was served is served again, bit for bit"""
    first, again = walk[state]
    for name in CALLS:
        a, b = first[name], again[name]
        if isinstance(a, str):
            assert a == b, (state, name, a, b)
            continue
        assert not isinstance(b, str) and len(a) == len(b), (state, name, b)
        for k, (x, y) in enumerate(zip(a, b)):
            assert x.shape == y.shape and x.dtype == y.dtype and np.array_equal(_bits(x), _bits(y)), (state, name, "field", k)


def test_a_refusal_reports_its_own_entry_point(walk):
    """rpe_last_error gives the text of the call that failed: rpe_fetch_results(0) used to return RPE_ERR_INVALID without
    one, and the caller read the refusal of the call before it"""
    first, second = walk["texts"]
    assert "rpe_fetch_structure" in first and NONE in first, first
    assert "rpe_fetch_results" in second and NONE not in second and "rpe_fetch_structure" not in second, second
