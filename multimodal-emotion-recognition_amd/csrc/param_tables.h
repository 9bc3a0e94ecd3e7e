// The parameter map of a configuration and every table cut from it (param_tables.hip): ONE host table per configuration - offsets,
// optimizer items, tile and slice prefixes - and ONE cache of the device copies the optimizer, norm and statistics kernels walk.
// Shared with the plan files (plan.h), which build their plans on the same map and their in-launch optimizer tables with the same helpers.
#pragma once
#include "../../include/m2fnet_hip.h"
#include "ops.h"

#include <cstdint>
#include <string>
#include <utility>
#include <vector>

namespace m2f {

// the thread's last error (m2f_last_error): fail() returns 1, hipfail() 2
int fail(const std::string& m);
int hipfail(hipError_t e, const char* what);
const char* last_error();
#define M2F_HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return ::m2f::hipfail(e_, #x); } while (0)
// the EMA entry points' own arguments (`what`: the entry point's name): a 16-byte aligned average buffer, ema_w = 1 - decay in [0, 1]
int ema_args_bad(const char* what, const float* ema, float ema_w);

// ---------------------------------------------------------------------------------------------------
// parameter map (mirror of layout.py / reference state_dict order)
// ---------------------------------------------------------------------------------------------------
struct EncLayerP { size_t in_w, in_b, out_w, out_b, l1_w, l1_b, l2_w, l2_b, n1_w, n1_b, n2_w, n2_b; };
struct ModalityP { std::vector<std::vector<EncLayerP>> enc; size_t norm_w = 0, norm_b = 0, proj_w = 0, proj_b = 0; };
struct FamP { size_t in_w, in_b, out_w, out_b, lin_w, lin_b; };
struct LinP { size_t w, b; };
struct ParamMap {
    ModalityP audio, text;
    std::vector<FamP> fam;
    std::vector<LinP> cls;               // Linear0, extra hidden..., last
    std::vector<int64_t> offsets, numels;
    size_t total = 0;
    struct Mat { size_t off; int rows, cols; size_t soff, soff_t; };   // 2-D tensors + offsets of their padded bf16 shadow
    std::vector<Mat> mats;                                             // and of the shadow of their transpose
    size_t shadow_elems = 0;
};
int cls_in_width(const m2f_config& c);
int check_config(const m2f_config& c);
int build_param_map(const m2f_config& c, ParamMap& pm);

// ---------------------------------------------------------------------------------------------------
// the host table of a configuration: built once per distinct m2f_config, kept for the life of the process, touches no device
// ---------------------------------------------------------------------------------------------------
constexpr int64_t ADAM_TABLE_BYTES = 64 * 1024;          // behind the shadows: AdamItem[n] | int tile_begin[n + 1]
struct ParamTable {
    m2f_config cfg;
    std::vector<int64_t> offsets, numels;    // first element / element count of tensor i
    size_t total = 0;
    size_t shadow_elems = 0;                 // bf16 elements of the shadows, rounded to 128: the 64 KB table region starts there
    std::vector<AdamItem> items;             // item i = tensor i, tile_begin absolute (m2f_launch_adam_shadowed walks them)
    std::vector<int> tile_begin;             // [n + 1]
    std::vector<int> slice_begin;            // [n + 1]: first M2F_PARAM_SLICE slice of tensor i
    bool items_fit = false;                  // the items fit the table region and M2F_ADAM_MAX_ITEMS
    int n() const { return (int)offsets.size(); }
};
// -> the table, or null (last error set).  need_items: also refuse a configuration whose items do not fit the region behind the shadows
const ParamTable* param_table(const m2f_config& cfg, bool need_items = false);
// the tensor that holds element `e` of the flat buffers (or the pad behind it); -1: before the first
int tensor_at(const ParamTable& t, long long e);

// a tensor -> group map (`what`: the entry point's name): one entry per tensor, each -1 (no group) .. M2F_ADAM_MAX_GROUPS - 1
int group_map_bad(const char* what, const ParamTable& t, const int* tensor_group, int n_tensors);

// tiles of an item: 64 x 64 tiles of a matrix / 4096-element tiles of a 1-D run; flat: 4096-element tiles of all its elements
int item_tiles(const AdamItem& it, bool flat = false);
// Renumbers items[].tile_begin from 0 -> the number of tiles; tile_begin = the n + 1 prefix.  groups (optional, parallel to items):
// items whose group is < 0 are dropped first, from both lists.
int retile(std::vector<AdamItem>& items, std::vector<int>* groups, bool flat, std::vector<int>& tile_begin);

// One hipMalloc (freeing what `dev` held) for the host arrays `sec` (pointer, bytes), each on a 256-byte boundary and copied with
// one hipMemcpy, 256 bytes of slack behind the last; at[i] = device address of section i.
int upload_packed(void*& dev, const std::vector<std::pair<const void*, size_t>>& sec, std::vector<char*>& at);

}  // namespace m2f
