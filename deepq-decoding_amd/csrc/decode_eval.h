// The scoring handle of include/deepq_hip.h (dq_decode_eval_create): shared by decode_eval.hip (sampler, verdict, counters) and match_st.hip (the
// space-time matching baseline, whose tables the handle owns).
#pragma once
#include "common.h"

struct MatchStTables;                                            // match_st.hip: distance and path tables of the matching decoder, on the device
void match_st_free(MatchStTables* t);

struct dq_decode_eval {
    int d, depth, model, use_Y, max_volumes;
    DqRateTable rates;          // per-volume thresholds of a sample call (2 max_volumes + 2 words)
    // the Dense-stack referee's pass (allocated at its first use): the residuals' planes as two-word records (padded: the pass reads word 8 of a
    // record), "no move" actions, the classes
    u64* xz;
    int32_t* no_action;
    u8* dec;
    MatchStTables* match_st;    // dq_decode_match's / dq_env_match_select's tables (built and uploaded at the first call of either)
};

dq_status match_st_tables(dq_decode_eval* V);                    // match_st.hip: builds V->match_st unless it is there
