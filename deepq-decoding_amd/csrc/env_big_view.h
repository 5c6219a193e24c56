// A read-only view of the wide environment's lattice records for kernels outside env_big.hip (env_wide_uf.hip): the wide twin of env_dev.h's EnvStateView /
// env_state_view.  The record's layout is env_big.hip's header comment: x[W] z[W] acted[W] round meta completed[LW] legal[LW] volume[depth][W].
#pragma once
#include "common.h"

struct dq_envb;

struct EnvbStateView {
    const u64* state;           // [n_envs][sw]
    int sw, W, LW, n_envs, d, depth, model, use_Y, identity, n_actions;
    u32 env_id_base;
};
dq_status envb_state_view(const dq_envb* E, EnvbStateView* v);
