// rpe_host.h -- the host helpers rpe_api.hip and rpe_features.hip share.  Declarations only: each has its one definition,
// and its comment, in rpe_api.hip.
#pragma once
#include "rpe_internal.h"

// argument heads, each with its one message
int check_batch(rpe_handle *h, int B);
int check_desc_counts(rpe_handle *h, const int32_t *n, int B);
int check_match_counts(rpe_handle *h, const int32_t *m, int B);
int check_positive(rpe_handle *h, const char *who, const char *name, double v);
bool all_finite(const double *v, size_t n);
int check_cameras(rpe_handle *h, const rpe_camera *c, int n, const char *who);
int l2_desc_bytes(rpe_handle *h, const float *h_desc1, const int32_t *n1, const float *h_desc2, const int32_t *n2, int B, std::vector<uint8_t> &u);

// the fetch (dst != NULL; one wait) and the upload (src != NULL and bytes > 0; no wait), on the handle's stream
struct Copy { void *dst; const void *src; size_t bytes; };
int fetch(rpe_handle *h, std::initializer_list<Copy> pieces);
int upload(rpe_handle *h, std::initializer_list<Copy> pieces);
int upload_counts(rpe_handle *h, const int32_t *n1, const int32_t *n2, int B);
int upload_descriptors(rpe_handle *h, const uint8_t *h_desc1, const uint8_t *h_desc2, int B);
int set_K(rpe_handle *h, const double K[9]);

// the last run: its gate (the table is at the definition), the first B pairs of it, its structure buffers made current,
// and the end of its claim on the per-match buffers.  Every write to h->last stays in rpe_api.hip.
enum : unsigned { NEED_UNCHUNKED = 1, NEED_PER_MATCH = 2, NEED_COUNT = 4, NEED_TABLE = 8 };
int last_run_gate(rpe_handle *h, const char *who, int n, unsigned needs);
RpeRun last_run_first(const rpe_handle *h, int B);
int last_run_structure(rpe_handle *h, int B, bool always);
void last_run_end(rpe_handle *h, bool images_too = false);

// head of the geometry stage calls: capacity, cameras, points and intrinsics resident; `run` is the stage run over the B pairs
int stage_begin(rpe_handle *h, const char *who, const float *p1, const float *p2, const int32_t *m, int B,
                const double *K, const rpe_camera *cam1, const rpe_camera *cam2, RpeRun &run);
