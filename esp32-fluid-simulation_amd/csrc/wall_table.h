// wall_table.h -- the wall table of include/sfl.h "WALL VELOCITIES" as the host forms it, for batches (walls.cpp) and
// contexts (context_walls.cpp) alike: the records checked against the code bytes of the mask that is set, split into rows,
// of two records on one cell the later kept, each row in cell order, and the rows laid out as ONE CSR table with a row per
// member -- batch.h BatchProfile's layout; a table all members share is written out once per member.  Plain C++: no HIP,
// no handle, nothing allocated but vectors, so that tests/cpp/walls_driver.cpp holds it to its rule on its own.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace sfl {
namespace walls {

struct Record {
    uint32_t cell;   // dim_x * j + i
    float u, v;      // bits as given
};
typedef std::vector<std::vector<Record>> Rows;   // one row for all members, or one per member

// What is wrong with the first record that may not be staged: nothing (record < 0), a cell outside the grid, or a cell
// that is fluid in member `member`'s mask.
struct Offence {
    enum Kind { kNone, kOutside, kFluid } kind = kNone;
    int record = -1, member = 0, i = 0, j = 0;
};

// The records against the mask.  codes: the solids' code bytes (bit 4 = the cell is fluid), `members` masks of dim_x *
// dim_y bytes when per_member, else one.  who: the member of every record, or null = every record goes to every member.
inline Offence first_offence(const int *who, const int *cells_ij, int n, int dim_x, int dim_y, const uint8_t *codes, bool per_member, int members)
{
    const size_t cells = (size_t)dim_x * (size_t)dim_y;
    for (int k = 0; k < n; ++k) {
        const int i = cells_ij[2 * k], j = cells_ij[2 * k + 1];
        Offence bad;
        bad.record = k;
        bad.i = i;
        bad.j = j;
        if (i < 0 || i >= dim_x || j < 0 || j >= dim_y) {
            bad.kind = Offence::kOutside;
            return bad;
        }
        const size_t c = (size_t)j * dim_x + i;
        const int m0 = who ? who[k] : 0, m1 = who ? who[k] + 1 : (per_member ? members : 1);
        for (int m = m0; m < m1; ++m)
            if (codes[(per_member ? (size_t)m * cells : 0) + c] & 16) {
                bad.kind = Offence::kFluid;
                bad.member = m;
                return bad;
            }
    }
    return Offence{};
}

// the records of one row sorted by cell, of two on one cell the later kept
inline void unique_by_cell(std::vector<Record> &row)
{
    std::stable_sort(row.begin(), row.end(), [](const Record &a, const Record &b) { return a.cell < b.cell; });
    size_t n = 0;
    for (size_t k = 0; k < row.size(); ++k) {
        if (k + 1 < row.size() && row[k + 1].cell == row[k].cell) continue;
        row[n++] = row[k];
    }
    row.resize(n);
}

// The rows of n checked records: one (who == null) or `members` of them, duplicates removed, in cell order.
inline Rows rows_of(const int *who, const int *cells_ij, const float *vel_xy, int n, int dim_x, int members)
{
    Rows rows(who ? (size_t)members : 1);
    for (int k = 0; k < n; ++k)
        rows[who ? who[k] : 0].push_back(Record{(uint32_t)(cells_ij[2 * k + 1] * dim_x + cells_ij[2 * k]), vel_xy[2 * k], vel_xy[2 * k + 1]});
    for (std::vector<Record> &row : rows) unique_by_cell(row);
    return rows;
}

// ONE CSR table with a row per member: member m's records are [offsets[m], offsets[m + 1]).  ok: the records over all
// members fit an int.
struct Table {
    std::vector<int> offsets;
    std::vector<uint32_t> cells;
    std::vector<float> vel;
    bool ok = true;
};
inline Table table_of(const Rows &rows, int members)
{
    Table t;
    t.offsets.assign((size_t)members + 1, 0);
    const bool shared = rows.size() == 1 && members != 1;
    for (int m = 0; m < members; ++m) {
        for (const Record &r : rows[shared ? 0 : (size_t)m]) {
            t.cells.push_back(r.cell);
            t.vel.push_back(r.u);
            t.vel.push_back(r.v);
        }
        if (t.cells.size() > (size_t)INT32_MAX) {
            t.ok = false;
            return t;
        }
        t.offsets[(size_t)m + 1] = (int)t.cells.size();
    }
    return t;
}

// the records a table holds, a shared row counted once per member
inline int64_t records_held(const Rows &rows, int members)
{
    int64_t held = 0;
    for (const std::vector<Record> &row : rows) held += (int64_t)row.size() * (rows.size() == 1 ? members : 1);
    return held;
}

}  // namespace walls
}  // namespace sfl
