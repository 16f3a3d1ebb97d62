// vf_graph_handle.hpp -- the GraphManager handle (struct vf_graph) as the translation units behind its C ABI see it: vf_graph.cpp,
// which owns the bookkeeping, and vf_graph_scores.cpp, vf_graph_errors.cpp and vf_graph_robust.cpp, whose entry points need engine calls that vf_graph.cpp must not reference
// (the host tests link vf_graph.cpp against a stand-in engine that has only what vf_graph.cpp calls).  Internal: not installed,
// not part of include/vilfusion.h.  Host code, no HIP.
#pragma once

#include <atomic>
#include <cstdint>
#include <deque>
#include <mutex>
#include <utility>
#include <vector>

#include "../../include/vilfusion.h"

struct ImuSample { double t, acc[3], gyro[3]; };
struct PendingImu {            // one queued CombinedImuFactor (GraphManager::_imuQueue)
    uint64_t key;              // X(key-1) -> X(key)
    std::vector<double> steps; // 7 per step: dt, acc, gyro
    double bias[6];            // getBias() at reserveNode time (GraphManager.cpp:61)
    std::vector<double> record; // non-empty: a ready-made factor handed in through vf_add_imu_factor (addFactor), 190 doubles
    bool staged = false;        // preintegrated on the device already, at reserveNode time (where the reference preintegrates: GraphManager.cpp:59-66)
};
// (loss, loss_k: the robust loss of a band factor, vf_add_between_robust; a Gaussian factor by default)
// (kind: VF_ABSOLUTE_NONE for a between factor; an absolute factor on key b, vf_add_absolute_pose / _position, is staged like a band
// factor from b - 1 -- it takes b's band slot -- and goes to the engine through vf_engine_set_absolute)
struct PendingBetween { uint64_t a, b; double rec[VF_BTW_RECORD]; bool on_device = false; int loss = VF_LOSS_NONE; double loss_k = 0.0; int kind = VF_ABSOLUTE_NONE; };
// a between factor as the caller handed it in: what GraphManager::graph() shows until the next solve (vf_graph_get_staged, vf_graph_get_staged_loss)
// (kind: as PendingBetween's; an absolute factor shows a = b = its key, a position fix its 3 x 3 covariance in the translation block of cov)
struct StagedFactor { uint64_t a, b; double q[4], t[3], cov[36]; int loss = VF_LOSS_NONE; double loss_k = 0.0; int kind = VF_ABSOLUTE_NONE; };
typedef int (*vf_between_loss_setter)(vf_engine*, int, int, const int32_t*, const int32_t*, const double*);   // vf_engine_set_between_loss
// ... and the two calls a far factor's loss needs: vf_engine_set_extra_between_robust, vf_engine_get_extra_between_loss
typedef int (*vf_far_robust_setter)(vf_engine*, int, int, const int32_t*, const int32_t*, const double*, const int32_t*, const double*);
typedef int (*vf_far_loss_getter)(vf_engine*, int, int32_t*, double*);
typedef int (*vf_absolute_setter)(vf_engine*, int, int, const int32_t*, const int32_t*, const double*);       // vf_engine_set_absolute
struct vf_robust_calls { vf_between_loss_setter set_between_loss; vf_far_robust_setter set_far_robust; vf_far_loss_getter get_far_loss; };

struct vf_graph {
    vf_engine* eng = nullptr;
    vf_graph_opts opts{};
    vf_imu_params imu{};
    // guarded by graph_mutex (GraphManager::_graphMutex + IMUManager::_bufferMutex)
    std::mutex graph_mutex, buffer_mutex;
    std::mutex solve_mutex;        // one vf_solve at a time (order: solve -> graph -> state; nothing else takes it)
    std::deque<ImuSample> buffer;
    std::deque<PendingImu> imu_queue;
    std::vector<PendingBetween> staged_between;
    // how the solve's staging step hands the losses of band factors to the engine, behind their records: null until the first robust
    // factor is added (vf_graph_robust.cpp hands it to vf_add_between_, which writes it under graph_mutex; a solve reads it under graph_mutex too,
    // in its take, with the factors; vf_graph.cpp never names the engine call), and nothing is called
    vf_between_loss_setter set_between_loss = nullptr;
    // ... and how it sends a far list whose entries carry losses, and reads the losses back with the list after a marginalisation
    // (robust_far below): set with set_between_loss, by the same hand, under the same rules
    vf_far_robust_setter set_far_robust = nullptr;
    vf_far_loss_getter get_far_loss = nullptr;
    // ... and how it hands absolute factors to the engine (vf_graph_absolute.cpp sets it with the first one, as above)
    vf_absolute_setter set_absolute = nullptr;
    bool robust_far = false;       // vf_set_robust_far: a pair the band cannot hold may carry a loss (guarded by graph_mutex)
    // Between factors the band cannot hold -- wider than VF_MAX_BANDWIDTH keyframes, or a second one ending at a key (loop
    // closures; iSAM2 takes any pair of keys, GraphManager.cpp:83-88): handed to the engine as "far" factors
    // (vf_engine_set_extra_between) at every solve.  When the older key of one leaves the fixed-lag window the engine
    // marginalises the factor with it and keeps it from then on as linear rows of its own (include/vilfusion.h): the entry
    // here goes (the list is replaced by what vf_engine_get_extra_between reports).  band_end[k] != 0: key k
    // already carries a band factor.  far_new counts the ones added since the last solve (they are part of graph()->size()).
    std::vector<PendingBetween> far_between;
    std::deque<uint8_t> band_end;      // entry i: key band_base + i (trimmed below the window at every solve)
    uint64_t band_base = 0;
    bool has_band_end(uint64_t k) const { return k >= band_base && k - band_base < band_end.size() && band_end[k - band_base]; }
    void set_band_end(uint64_t k, uint8_t v) {
        if (k < band_base) return;
        if (k - band_base >= band_end.size()) { if (!v) return; band_end.resize(k - band_base + 1, 0); }
        band_end[k - band_base] = v;
    }
    int far_new = 0;
    bool far_on_device = false;    // the engine holds a non-empty far list (written under solve_mutex only)
    std::atomic<int> far_linear{0};  // far ends of the engine's linear far factor (far factors marginalised with their older key): they share opts.max_far_factors
    int staged_count = 3;  // the three priors (GraphManager.cpp:33-35)
    bool priors_staged = true;              // ... which the first solve takes with everything else (_graph->resize(0), :114)
    std::vector<StagedFactor> staged_log;   // the between factors among them, in the order addBetweenFactor took them
    uint64_t current_key = 0;
    double last_pose_time = -1.0;
    std::vector<double> key_time;  // time of each reserved key
    // guarded by state_mutex (GraphManager::_stateMutex)
    std::mutex state_mutex;
    double state[16] = {1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    double anchor[16] = {1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};   // X(0), V(0), B(0) and the means of their priors
    uint64_t solved_key = 0;  // keys [0, solved_key] hold states on the device
    int lo = 0;               // slot of the oldest keyframe in the window
    uint64_t key_base = 0;    // slot = key - key_base (advances by multiples of 64 on compaction)
    std::vector<std::pair<vf_callback, void*>> callbacks;
    std::vector<std::pair<vf_cov_callback, void*>> cov_callbacks;
    bool solved_once = false;   // a vf_solve has succeeded
    bool cov_valid = false;     // the engine holds the covariances of the window as the last solve left it (vf_engine_marginals)
    bool cov_tail = false;      // ... of the last two keys only (VF_MARGINALS_TAIL, vf_graph_gate.cpp): whoever needs more computes the full ones
    bool cov_pose = false;      // ... computed with VF_MARGINALS_POSE: the nav_msgs records are there too (vf_graph_scores.cpp)
    bool err_valid = false;     // the engine holds the per-factor errors of the window as the last solve left it (vf_graph_errors.cpp)
};

// vf_add_between with a loss (vf_graph.cpp): VF_LOSS_NONE is vf_add_between itself; any other loss is for band factors only unless
// vf_set_robust_far has switched far losses on.  calls: the engine calls a loss needs (null with VF_LOSS_NONE), kept in the handle
extern "C" int vf_add_between_(vf_graph* g, uint64_t prev, uint64_t cur, const double q[4], const double t[3], const double cov[36], int loss, double loss_k,
                               const vf_robust_calls* calls);
// an absolute factor on `key` (vf_graph.cpp; vf_graph_absolute.cpp has built and checked the record, the loss and what graph() shows)
extern "C" int vf_add_absolute_(vf_graph* g, uint64_t key, int kind, const double rec[VF_BTW_RECORD], const StagedFactor* shown, int loss, double loss_k,
                                vf_absolute_setter setter, const vf_robust_calls* calls);
extern "C" int vf_between_record_(const double q[4], const double t[3], const double cov[36], double rec[VF_BTW_RECORD]);   // vf_graph.cpp

// key -> keyframe slot of the handle's one window, and the oldest key still in it
static inline int slot_of(const vf_graph* g, uint64_t key) { return (int)(key - g->key_base); }
static inline uint64_t oldest_key(const vf_graph* g) { return g->key_base + (uint64_t)g->lo; }
