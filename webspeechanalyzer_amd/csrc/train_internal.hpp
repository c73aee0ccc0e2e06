// train_internal.hpp — what train.hip (the solo trainer) and train_group.hip (K7g) share on the host: wsa_trainer, the workgroup count
// of a stage, the order of an epoch's launches, and the checking and staging of an epoch's order.  Internal to csrc/.
#pragma once
#include <cstring>
#include <string>
#include <vector>
#include "host_plan.hpp"
#include "train_stages.hpp"

struct wsa_trainer {
    wsa_ctx* ctx = nullptr;
    wsa_train_group* group = nullptr;                          // the living group that has adopted this trainer, if any
    wsa_train::TrainDesc desc = {};                            // all the stages read; its buffers are the arena's
    uint32_t n_rows = 0, mcap = 0, epoch = 0;                  // mcap: rows of a[l] and dz, the larger of batch and n_val, padded
    uint32_t* h_order[2] = {}; hipEvent_t ev[2] = {};          // pinned staging of the order, two epochs deep
    std::vector<double> in_min, in_max;
    std::vector<std::string> labels; bool has_labels = false;
    wsa::DevArena mem;
};

namespace wsa_train {

void tg_orphan(wsa_train_group* g);                            // train_group.hip: a member is destroyed before its group

enum TrStage { TR_FORWARD, TR_LOSS, TR_BACKWARD, TR_UPDATE, TR_FINISH };

inline uint32_t up16(uint32_t v) { return (v + 15u) & ~15u; }

// the workgroups of one trainer in the launch of `stage` at position `pos` of `step` (or of the validation pass): one wave per tile,
// TR_WAVES tiles per workgroup; 0 when the trainer has dropped out of the epoch by `step` or has no layer at `pos`
inline uint32_t stage_blocks(const TrainDesc& t, TrStage stage, uint32_t step, int pos) {
    if (stage == TR_FINISH) return 1;
    if (step == TR_VALIDATION ? t.n_val == 0 : t.n_steps <= step) return 0;
    const uint64_t rb = tr_step(t, step, nullptr).mp / 16;
    const int l = stage == TR_FORWARD ? pos : t.nl - 1 - pos;                // the trainer's layer at this position
    uint64_t tiles = 0;
    switch (stage) {
        case TR_FORWARD: if (l < t.nl) tiles = rb * (t.pad[l + 1] / 16); break;
        case TR_LOSS: return 1;
        case TR_BACKWARD: if (l > 0) tiles = rb * (t.pad[l] / 16); break;
        case TR_UPDATE: if (l >= 0) tiles = (uint64_t)(t.pad[l] / 16 + 1) * (t.pad[l + 1] / 16); break;
        case TR_FINISH: break;
    }
    return (uint32_t)((tiles + TR_WAVES - 1) / TR_WAVES);
}

// The order of an epoch's launches, for one trainer or a group stepped in lock step, from the members' shapes alone: emit(stage, step,
// pos) is called once per launch, in the order the launches go out.  Returns their number, which is TG-1's formula: 3 lmax per step
// (lmax: the most layers among the members still in the epoch), lval + 1 for the validation pass, 1 for the finish.
template <typename Emit>
uint64_t group_plan(const uint32_t* nl, const uint32_t* n_steps, const uint32_t* n_val, uint32_t n, Emit emit) {
    uint32_t longest = 0, lval = 0;
    for (uint32_t i = 0; i < n; i++) { if (n_steps[i] > longest) longest = n_steps[i]; if (n_val[i] && nl[i] > lval) lval = nl[i]; }
    uint64_t launches = 0;
    const auto out = [&](TrStage stage, uint32_t step, uint32_t pos) { emit(stage, step, (int)pos); launches++; };
    const auto forward_and_loss = [&](uint32_t step, uint32_t lmax) {
        for (uint32_t l = 0; l < lmax; l++) out(TR_FORWARD, step, l);
        out(TR_LOSS, step, 0);
    };
    for (uint32_t step = 0; step < longest; step++) {
        uint32_t lmax = 0;
        for (uint32_t i = 0; i < n; i++) if (n_steps[i] > step && nl[i] > lmax) lmax = nl[i];
        forward_and_loss(step, lmax);
        for (uint32_t j = 0; j < lmax; j++) {                                // a layer's backward reads its weights: before their update
            if (j + 1 < lmax) out(TR_BACKWARD, step, j);
            out(TR_UPDATE, step, j);
        }
    }
    if (lval) forward_and_loss(TR_VALIDATION, lval);                         // the same forward over the validation rows, after the last update
    out(TR_FINISH, 0, 0);
    return launches;
}

// the same over trainers: the epoch of members[0 .. n-1]
template <typename Emit>
uint64_t group_plan(wsa_trainer* const* members, uint32_t n, Emit emit) {
    uint32_t nl[WSA_TRAIN_GROUP_MAX], n_steps[WSA_TRAIN_GROUP_MAX], n_val[WSA_TRAIN_GROUP_MAX];
    for (uint32_t i = 0; i < n; i++) { nl[i] = (uint32_t)members[i]->desc.nl; n_steps[i] = members[i]->desc.n_steps; n_val[i] = members[i]->desc.n_val; }
    return group_plan(nl, n_steps, n_val, n, emit);
}

inline void count_only(TrStage, uint32_t, int) {}                            // group_plan's emitter when only the count is wanted

// "" or why `order` (not NULL) is refused: an entry outside the training rows
inline std::string order_refusal(const wsa_trainer* t, const uint32_t* order) {
    const uint32_t n_train = t->desc.n_train;
    for (uint32_t i = 0; i < n_train; i++)
        if (order[i] >= n_train) return "order[" + std::to_string(i) + "] = " + std::to_string(order[i]) + " is outside 0 .. " + std::to_string(n_train - 1);
    return "";
}

// the epoch's order through the trainer's pinned staging (two epochs deep) into desc.order, on s
inline wsa_status stage_order(wsa_trainer* t, const uint32_t* order, hipStream_t s) {
    wsa_ctx* ctx = t->ctx;
    const size_t bytes = (size_t)t->desc.n_train * sizeof(uint32_t);
    const int slot = t->epoch & 1;                                           // the copy that last read this staging buffer is two epochs back
    HIP_TRY(ctx, hipEventSynchronize(t->ev[slot]));
    std::memcpy(t->h_order[slot], order, bytes);
    HIP_TRY(ctx, hipMemcpyAsync(t->desc.order, t->h_order[slot], bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipEventRecord(t->ev[slot], s));
    return WSA_OK;
}

}  // namespace wsa_train
