// train_group.hip — K7g: K7's stages for a GROUP of trainers stepped in lock step (specification TG-1), and wsa_train_group_*
// of the C ABI (include/wsa.h "Training groups").  One launch covers one stage of every member that has that stage in this step.  Whole
// workgroups belong to one member: member i owns workgroups prefix[i] .. prefix[i + 1] - 1 (none when it has dropped out of the epoch
// or has no layer at this position), its workgroup's index within its part is blockIdx.x - prefix[i], and from there on the solo
// kernel's body (train_stages.hpp) runs on parameters built, by the functions the solo trainer calls on the host, from the member's row
// of the description table (device memory, written once at wsa_train_group_create) and the launch's step and position.  Members share
// no buffer, no sum crosses a workgroup: a member's bits are its solo run's.  The loss and the update each have ONE grouped kernel that
// takes the member's kind (softmax + SGD, or mean squared error + Adam) from its description, so a step of a mixed group still costs
// 3 . max nl launches.
#include <string>
#include <vector>
#include "train_internal.hpp"

using wsa_api::fail;
using namespace wsa_train;

namespace {

constexpr int TG_MAX = WSA_TRAIN_GROUP_MAX;

// by value, 37 words: the workgroup-count prefix over the members, the step (or TR_VALIDATION), bit i of order_mask set when member i
// reads its rows through its order buffer in this epoch (clear: the identity), and the layer position of the launch
struct TgLaunch { uint32_t prefix[TG_MAX + 1]; uint32_t n, step, order_mask; int pos; };

__device__ __forceinline__ uint32_t tg_member_of(const TgLaunch& g, uint32_t block) {    // uniform over the workgroup
    uint32_t i = 0;
    while (i + 1 < g.n && block >= g.prefix[i + 1]) i++;
    return i;
}

__device__ __forceinline__ TrStep tg_step(const TrainDesc& t, const TgLaunch& g, uint32_t i) {
    return tr_step(t, g.step, (g.order_mask >> i) & 1u ? t.order : t.identity);
}

__global__ void __launch_bounds__(TR_THREADS) train_group_forward_kernel(const TrainDesc* tab, TgLaunch g) {   // g.pos: the layer
    const uint32_t i = tg_member_of(g, blockIdx.x);
    const TrainDesc& t = tab[i];
    tr_forward_body(tr_forward_params(t, tg_step(t, g, i), g.pos), blockIdx.x - g.prefix[i]);
}

__global__ void __launch_bounds__(TR_LOSS_THREADS) train_group_loss_kernel(const TrainDesc* tab, TgLaunch g) {   // one workgroup per member
    __shared__ double s_loss[TR_LOSS_THREADS];
    __shared__ uint32_t s_hit[TR_LOSS_THREADS];
    const uint32_t i = tg_member_of(g, blockIdx.x);
    const TrainDesc& t = tab[i];
    const TrStep s = tg_step(t, g, i);
    if (t.regress) tr_loss_mse_body(tr_loss_mse_params(t, s), s_loss, s_hit);
    else tr_loss_body(tr_loss_params(t, s), s_loss, s_hit);
}

// g.pos: the position j of the backward / update stages; the host gives a member that has no layer there no workgroup
__global__ void __launch_bounds__(TR_THREADS) train_group_backward_kernel(const TrainDesc* tab, TgLaunch g) {
    const uint32_t i = tg_member_of(g, blockIdx.x);
    const TrainDesc& t = tab[i];
    tr_backward_body(tr_backward_params(t, tg_step(t, g, i), g.pos), blockIdx.x - g.prefix[i]);
}

__global__ void __launch_bounds__(TR_THREADS) train_group_update_kernel(const TrainDesc* tab, TgLaunch g) {
    const uint32_t i = tg_member_of(g, blockIdx.x);
    const TrainDesc& t = tab[i];
    const TrUpd u = tr_update_params(t, tg_step(t, g, i), g.pos);
    if (t.regress) tr_update_body<TrAdam>(tr_update_adam_params(t, u, g.pos), blockIdx.x - g.prefix[i]);
    else tr_update_body<TrSgd>(u, blockIdx.x - g.prefix[i]);
}

struct TgFinish { uint32_t epoch[TG_MAX]; };                                // by value: the epoch each member has just finished

__global__ void __launch_bounds__(TR_FINISH_THREADS) train_group_finish_kernel(const TrainDesc* tab, TgFinish g) {   // workgroup i: member i
    __shared__ double s_loss[TR_FINISH_THREADS];
    __shared__ uint32_t s_hit[TR_FINISH_THREADS];
    tr_finish_body(tr_finish_params(tab[blockIdx.x], g.epoch[blockIdx.x]), s_loss, s_hit);
}

}  // namespace

struct wsa_train_group {
    wsa_ctx* ctx = nullptr;
    uint32_t n = 0;
    wsa_trainer* member[WSA_TRAIN_GROUP_MAX] = {};
    TrainDesc* d_tab = nullptr;                                // the members' descriptions: all the group owns
    wsa::DevArena mem;
};

// a member is being destroyed before its group: the table points at its buffers, so the group lets go of every member and is empty
void wsa_train::tg_orphan(wsa_train_group* g) {
    for (uint32_t i = 0; i < g->n; i++) g->member[i]->group = nullptr;
    g->n = 0;
}

namespace {

// one grouped launch: the prefix of workgroup counts over the members that have `stage` at `pos` in `step`, then the kernel
void tg_launch(wsa_train_group* g, TrStage stage, uint32_t step, int pos, uint32_t order_mask, hipStream_t s) {
    if (stage == TR_FINISH) {
        TgFinish f{};
        for (uint32_t i = 0; i < g->n; i++) f.epoch[i] = ++g->member[i]->epoch;
        hipLaunchKernelGGL(train_group_finish_kernel, dim3(g->n), dim3(TR_FINISH_THREADS), 0, s, g->d_tab, f);
        return;
    }
    TgLaunch a{};
    a.n = g->n; a.step = step; a.order_mask = order_mask; a.pos = pos;
    for (uint32_t i = 0; i < g->n; i++) a.prefix[i + 1] = a.prefix[i] + stage_blocks(g->member[i]->desc, stage, step, pos);
    for (uint32_t i = g->n; i < WSA_TRAIN_GROUP_MAX; i++) a.prefix[i + 1] = a.prefix[i];
    const dim3 grid(a.prefix[g->n]);
    if (grid.x == 0) return;
    switch (stage) {
        case TR_FORWARD: hipLaunchKernelGGL(train_group_forward_kernel, grid, dim3(TR_THREADS), 0, s, g->d_tab, a); break;
        case TR_LOSS: hipLaunchKernelGGL(train_group_loss_kernel, grid, dim3(TR_LOSS_THREADS), 0, s, g->d_tab, a); break;
        case TR_BACKWARD: hipLaunchKernelGGL(train_group_backward_kernel, grid, dim3(TR_THREADS), 0, s, g->d_tab, a); break;
        case TR_UPDATE: hipLaunchKernelGGL(train_group_update_kernel, grid, dim3(TR_THREADS), 0, s, g->d_tab, a); break;
        case TR_FINISH: break;
    }
}

}  // namespace

extern "C" {

wsa_status wsa_train_group_launch_count(const uint32_t* nl, const uint32_t* n_train, const uint32_t* batch, const uint32_t* n_val,
                                        uint32_t n, uint64_t* per_epoch) {
    if (!nl || !n_train || !batch || !n_val || !per_epoch || n == 0 || n > WSA_TRAIN_GROUP_MAX) return WSA_ERR_INVALID;
    uint32_t steps[WSA_TRAIN_GROUP_MAX];
    for (uint32_t i = 0; i < n; i++) {
        if (nl[i] < 1 || nl[i] > WSA_MODEL_MAX_LAYERS || n_train[i] == 0 || batch[i] == 0) return WSA_ERR_INVALID;
        const uint32_t b = batch[i] < n_train[i] ? batch[i] : n_train[i];
        steps[i] = (n_train[i] + b - 1) / b;
    }
    *per_epoch = group_plan(nl, steps, n_val, n, count_only);
    return WSA_OK;
}

wsa_status wsa_train_group_create(wsa_ctx* ctx, wsa_trainer* const* members, uint32_t n, wsa_train_group** out) {
    if (!ctx || !members || !out) return fail(ctx, WSA_ERR_INVALID, "null argument");
    *out = nullptr;
    if (n == 0 || n > WSA_TRAIN_GROUP_MAX) return fail(ctx, WSA_ERR_INVALID, "a training group has 1 .. " + std::to_string(WSA_TRAIN_GROUP_MAX) + " members, got " + std::to_string(n));
    for (uint32_t i = 0; i < n; i++) {
        const std::string who = "member " + std::to_string(i);
        if (!members[i]) return fail(ctx, WSA_ERR_INVALID, who + " is NULL");
        if (members[i]->ctx != ctx) return fail(ctx, WSA_ERR_INVALID, who + " belongs to another context");
        for (uint32_t j = 0; j < i; j++)
            if (members[j] == members[i]) return fail(ctx, WSA_ERR_INVALID, who + " is the same trainer as member " + std::to_string(j));
        if (members[i]->group) return fail(ctx, WSA_ERR_INVALID, who + " is already in a living group");
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::vector<TrainDesc> tab(n);
    for (uint32_t i = 0; i < n; i++) tab[i] = members[i]->desc;
    wsa_train_group* g = new wsa_train_group();
    g->ctx = ctx; g->n = n;
    if (!g->mem.upload(&g->d_tab, tab)) {
        const std::string msg = std::string("device allocation / copy failed: ") + hipGetErrorString(hipGetLastError());
        delete g;
        return fail(ctx, WSA_ERR_HIP, msg);
    }
    for (uint32_t i = 0; i < n; i++) { g->member[i] = members[i]; members[i]->group = g; }
    *out = g;
    return WSA_OK;
}

void wsa_train_group_destroy(wsa_train_group* g) {
    if (!g) return;
    (void)hipSetDevice(g->ctx->device);
    (void)hipDeviceSynchronize();                                            // launches still in flight read the table
    for (uint32_t i = 0; i < g->n; i++) g->member[i]->group = nullptr;
    delete g;
}

wsa_status wsa_train_group_epoch(wsa_train_group* g, const uint32_t* const* orders, void* stream) {
    if (!g) return WSA_ERR_INVALID;
    wsa_ctx* ctx = g->ctx;
    if (g->n == 0) return fail(ctx, WSA_ERR_INVALID, "a member of the group was destroyed before the group: the group is empty");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    for (uint32_t i = 0; orders && i < g->n; i++) {                          // every member's order before anything is enqueued
        if (!orders[i]) continue;
        const std::string why = order_refusal(g->member[i], orders[i]);
        if (!why.empty()) return fail(ctx, WSA_ERR_INVALID, "member " + std::to_string(i) + ": " + why);
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    uint32_t order_mask = 0;
    for (uint32_t i = 0; orders && i < g->n; i++) {
        if (!orders[i]) continue;
        const wsa_status st = stage_order(g->member[i], orders[i], s);
        if (st != WSA_OK) return st;
        order_mask |= 1u << i;
    }
    group_plan(g->member, g->n, [&](TrStage stage, uint32_t step, int pos) { tg_launch(g, stage, step, pos, order_mask, s); });
    HIP_TRY(ctx, hipGetLastError());
    return WSA_OK;
}

wsa_status wsa_train_group_stats(wsa_train_group* g, void* stream, wsa_train_stats* out) {
    if (!g) return WSA_ERR_INVALID;
    wsa_ctx* ctx = g->ctx;
    if (!out) return fail(ctx, WSA_ERR_INVALID, "null argument");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    for (uint32_t i = 0; i < g->n; i++)
        HIP_TRY(ctx, hipMemcpyAsync(out + i, g->member[i]->desc.stats, sizeof(wsa_train_stats), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    return WSA_OK;
}

wsa_status wsa_train_group_launches(const wsa_train_group* g, uint32_t* per_epoch) {
    if (!g) return WSA_ERR_INVALID;
    if (!per_epoch) return fail(g->ctx, WSA_ERR_INVALID, "null argument");
    *per_epoch = (uint32_t)group_plan(g->member, g->n, count_only);
    return WSA_OK;
}

}  // extern "C"
