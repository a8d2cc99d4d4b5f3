// Internal glue between the optimiser, query, map and search translation units of libunevenhip.so (unevenhip.hip, traj_query.hip, map_build.hip, kino_search.hip).
#pragma once
#include <string>

#include "../../include/uneven_hip.h"
#include "uph_common.hpp"

namespace uph {
void setError(const std::string& s);
}

int uphMapDevice(const uph_map* m);
// grow-only device scratch owned by the map (slots 0..3), for the batched query entry points: no allocation per call once warm.
// One query at a time per map.  nullptr (with uph_last_error set) when the allocation fails.
void* uphMapScratch(uph_map* m, int slot, size_t bytes);
struct UphPtr {                 // non-owning view of a scratch slot
    void* p = nullptr;
    template <class T> T* as() { return (T*)p; }
};
uph::GridDev uphMapGrid(const uph_map* m);
// device occupancy layers of the map (uneven_map.cpp:170-179): occ [ncell], occ_r2 [nx * ny]; read by the front-end search (kino_search.hip)
void uphMapOcc(const uph_map* m, const char** occ, const char** occ_r2);
// how often the occupancy layers have been written (every launch of the two commit kernels of map_build.hip counts once): the stamp of a body layer
unsigned long long uphMapOccVersion(const uph_map* m);
// the body layer (body_occ.hip) as the search reads it: its map, its device bytes [nx][ny][nyaw], whether it was made from the map's occupancy as it is
// now, and the count of search contexts that name it (uph_body_layer_destroy refuses while it is not zero)
const uph_map* uphBodyLayerMap(const uph_body_layer* l);
const char* uphBodyLayerBytes(const uph_body_layer* l);
bool uphBodyLayerFresh(const uph_body_layer* l);
void uphBodyLayerUse(uph_body_layer* l, int delta);
// what the clearance layer (clearance.hip) needs of the body layer it is made from: the device it lives on, its dimensions, its write count (build, update and
// set count one each), and the count of clearance layers that name it (uph_body_layer_destroy refuses while it is not zero)
int uphBodyLayerDevice(const uph_body_layer* l);
void uphBodyLayerDims(const uph_body_layer* l, int dims3[3]);
unsigned long long uphBodyLayerWrites(const uph_body_layer* l);
void uphBodyLayerDepend(uph_body_layer* l, int delta);
// the clearance layer as the query (traj_query.hip) reads it: its body layer, its device values [nx][ny][nyaw], whether it was made from the body layer's bytes
// as they are now
const uph_body_layer* uphClearanceBody(const uph_clearance* l);
const unsigned short* uphClearanceValues(const uph_clearance* l);
bool uphClearanceFresh(const uph_clearance* l);
// the count of optimiser contexts that name the layer in a clearance term (uph_ctx_set_clearance_term; uph_clearance_destroy refuses while it is not zero)
void uphClearanceUse(uph_clearance* l, int delta);

// scope guards for the temporaries of the extern "C" entry points: every early return (HIPCHK) releases them
struct UphDevTmp {
    void* p = nullptr;
    ~UphDevTmp();
    template <class T> T* as() { return (T*)p; }
};
struct UphEventTmp {
    void* e = nullptr;          // hipEvent_t
    ~UphEventTmp();
};

// the front-end search (kino_search.hip) into its own device buffers, without the downloads of uph_kino_plan_batch: uph_plan_upload resamples the
// paths where the search left them.  out: device pointers into the context's buffers, valid until its next search -- paths [B][path_cap][3] (path_cap as passed),
// n_path [B] (may exceed path_cap: clipped), status [B] (UPH_KINO_*).  Blocking (the device is synchronised).
struct UphKinoOut {
    const double* paths = nullptr;
    const int* n_path = nullptr;
    const int* status = nullptr;
};
int uphKinoSearch(uph_kino* k, int32_t B, const double* starts, const double* goals, int32_t path_cap, int32_t max_expand, int32_t exp_cap, UphKinoOut& out);
const uph_map* uphKinoMap(const uph_kino* k);
