// The bodies of a plan family's entry points (<family>_workspace_bytes, <family>_op_run, <family>_run), written once for
// the ResNet forward and backward (backbone.hip, backbone_backward.hip) and the ConvNeXt, FocalNet and Swin families
// (through backbone_rows_core.h).  A family gives its op struct, its validation of one op without a launch (`need`
// receives the op's workspace bytes) and its launch of one op.
#pragma once

#include <algorithm>

#include "common.h"

namespace sdetr {
namespace {

template <class Op, int (*CheckOp)(const Op &, int, int64_t &), int (*RunOp)(hipStream_t, const Op &, int, void *, int64_t)>
struct Plan {
    static int64_t workspace_bytes(const Op *ops, int n_ops, int precision)
    {
        if (!ops || n_ops < 1) return -1;
        int64_t most = 0;
        for (int i = 0; i < n_ops; ++i) {
            int64_t need;
            if (CheckOp(ops[i], precision, need)) return -1;
            most = std::max(most, need);
        }
        return most;
    }

    static int op_run(const char *name, sdetr_stream_t stream, const Op *op, int precision, void *ws, int64_t ws_bytes)
    {
        if (!op) return fail("%s_op_run: null op", name);
        return RunOp((hipStream_t)stream, *op, precision, ws, ws_bytes);
    }

    static int run(const char *name, sdetr_stream_t stream, const Op *ops, int n_ops, int precision, void *ws, int64_t ws_bytes)
    {
        if (!ops || n_ops < 1) return fail("%s_run: empty plan", name);
        for (int i = 0; i < n_ops; ++i) {   // validate the whole plan before the first launch
            int64_t need;
            if (CheckOp(ops[i], precision, need)) return SDETR_EINVAL;
            if (need > ws_bytes || (need && !ws))
                return fail("%s_run: op %d needs %lld workspace bytes (workspace too small)", name, i, (long long)need);
        }
        for (int i = 0; i < n_ops; ++i)
            if (int rc = RunOp((hipStream_t)stream, ops[i], precision, ws, ws_bytes)) return rc;
        return 0;
    }
};

}  // namespace
}  // namespace sdetr
