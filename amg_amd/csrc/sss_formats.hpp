// sss_formats.hpp — host builders of the storage formats a matrix upload may choose (sss_formats.hip).
// Pure host code: no HIP runtime call, no kernel.  Each builder fills one plain struct with the
// arrays of its format exactly as they are stored in HBM (the formats: struct DevCSR).
#pragma once

#include "sss_engine.hpp"

namespace sss {

constexpr int kXellValueCap = 512;   // = kXellValues of the column ELL kernels (checked in sss_spmv.hip)

// Block dictionaries: pd[block] = {offset base, offset count, value base, value count} into dd / vd.
struct BlockDicts {
    std::vector<int4> pd;
    std::vector<int> dd;
    std::vector<double> vd;
    long long bytes() const   // what the kernels read of dd and vd
    {
        long long b = 0;
        for (const int4 &p : pd) b += 4LL * p.y + 8LL * p.w;
        return b;
    }
};
struct SortedTiles { HostBuf<unsigned> pk; HostBuf<double> pv; std::vector<int2> pb; };   // DevCSR::pk / pv / pb
struct SortedRows { HostBuf<int> ci; HostBuf<double> v; };   // ci / v with each row (segment) column-sorted
struct MergedGroups { std::vector<int> gp; HostBuf<unsigned> mk; HostBuf<double> mv; };   // DevCSR::mg_gp / mg_k / mg_v
struct DictTiles : BlockDicts { HostBuf<unsigned> code; };   // DevCSR::dv_code
struct ValueDict : BlockDicts { HostBuf<unsigned char> vi; };   // DevCSR::dv_vi (dd unused)
// DevCSR::dv_ell, W = ell_w; base: dv_ell_base (empty: offsets against the row index)
struct EllFormat : BlockDicts { HostBuf<unsigned char> ell; int W = 0; std::vector<int> base; };
// DevCSR::dv_xell with its own blocking (dd unused)
struct XellFormat : BlockDicts { std::vector<int> blk; HostBuf<unsigned> codes; };

int longest_row(const int *rp, int n);
// 256-row blocks (cut at the class split): the column ELL's blocking
int build_rows_blocks(int n, std::vector<int> &blk, int split);
bool build_sorted_tiles(const SSS_MAT &h, const std::vector<int> &blk, SortedTiles &out);
void sort_row_segments(const SSS_MAT &h, const int *seg, SortedRows &out);
void build_merged(const SSS_MAT &h, const int *seg, int G, MergedGroups &out);
bool build_dict_tiles(const SSS_MAT &h, const std::vector<int> &blk, DictTiles &out);
bool build_value_dict(const std::vector<int> &blk, const int *rp, const HostBuf<double> &pv, ValueDict &out);
// based: offsets against each row's first column (out.base) instead of the row index
bool build_ell(const SSS_MAT &h, const std::vector<int> &blk, bool based, EllFormat &out);
int xell_width(int L);         // row width for a longest row of L entries (0: none)
int xell_shift_for(int ncols); // column bits of a code (0: the columns do not fit)
bool build_xell(const SSS_MAT &h, int split, int W, int S, XellFormat &out);

}  // namespace sss
