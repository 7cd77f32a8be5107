// Lays a lens out for the near-field kernels on the host (metalens_amd/csrc/lens_pack.h), in the order ctx.hip does:
// the layout's part (ml_upload_layout: dense_collections, pack_ring_search, bin_cells, fit_lattice, lattice_records),
// then the tables' (the first synthesis: describe_table, locate_rings, classify_lens, pack_ring_tables,
// pack_centre_table).  Runs without a GPU.
//
//   lens_pack IN OUT
//
// Both files are a run of records, each a text line "NAME TYPE COUNT\n", COUNT items of TYPE in the machine's (little-
// endian) byte order, and a "\n".  TYPE is f8 (double), i4 (int32) or u1 (bytes).
//
// IN holds the arguments of the ml_upload_table calls and of ml_upload_layout as packing.pack_table and
// packing.pack_layout produce them, complex values as (re, im) pairs:
//   table<slot>.axis0 .axis1 .axis2 .order_k .values .bounds   f8   (slot 0 ... 31; centre.* for the centre table,
//   centre.periods f8[2] with it; .orders i4 is accepted and, as in the library, not read)
//   layout.B .r_center .period .lateral f8, layout.ring_gc i4, layout.cells f8[3 n_cells]
//   (layout.dphi .rot_table .tie_table .rot_center .rot_half are uploaded as they are: accepted, not read)
//   force_general, force_general_coll   i4[1]   the diagnostic build's two knobs (default 0)
// OUT holds every buffer the context would upload, under the name of its member of the context's Lens (common.h), and
// every scalar it would keep, under the name the kernel arguments give it: records (table_desc = TableDesc[33] with
// null pointers, coll = CollDesc[n_colls], ring_lutrec = RingBucket[], cell_lattice_rec = CellRec[]) as u1, scalars as
// arrays of one item.  After an error OUT holds error_code i4[1] and error_message u1[] alone.
// Build + run:  make -C tools lens_pack && tools/lens_pack lens.in lens.out
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#include "lens_pack.h"

using namespace ml;

struct Record {
    std::string type;
    std::vector<char> bytes;
    template <typename T>
    const T *as() const { return reinterpret_cast<const T *>(bytes.data()); }
    size_t count(size_t item) const { return bytes.size() / item; }
};

static FILE *g_out;

static void put(const char *name, const char *type, const void *data, size_t count, size_t item) {
    fprintf(g_out, "%s %s %zu\n", name, type, count);
    if (count) fwrite(data, item, count, g_out);
    fputc('\n', g_out);
}
static void put(const char *name, const std::vector<double> &v) { put(name, "f8", v.data(), v.size(), 8); }
static void put(const char *name, const std::vector<int32_t> &v) { put(name, "i4", v.data(), v.size(), 4); }
static void put(const char *name, double v) { put(name, "f8", &v, 1, 8); }
static void put(const char *name, int v) { put(name, "i4", &v, 1, 4); }

static int fail(const char *path, const PackError &e) {
    g_out = freopen(path, "wb", g_out);   // (drops what was written before the error)
    if (!g_out) return 1;
    put("error_code", e.code);
    put("error_message", "u1", e.msg.data(), e.msg.size(), 1);
    fclose(g_out);
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 3) return fprintf(stderr, "usage: %s IN OUT\n", argv[0]), 2;
    std::map<std::string, Record> in;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return perror(argv[1]), 2;
    char name[128], type[8];
    size_t count;
    while (fscanf(f, "%127s %7s %zu", name, type, &count) == 3) {
        const size_t item = type[1] - '0';
        Record &r = in[name];
        r.type = type;
        r.bytes.resize(count * item);
        if (fgetc(f) != '\n' || (count && fread(r.bytes.data(), item, count, f) != count) || fgetc(f) != '\n')
            return fprintf(stderr, "%s: record %s is cut short\n", argv[1], name), 2;
    }
    fclose(f);
    auto doubles = [&in](const std::string &n) {
        const Record &r = in[n];
        return std::vector<double>(r.as<double>(), r.as<double>() + r.count(8));
    };
    auto knob = [&in](const char *n) { return in.count(n) ? in[n].as<int32_t>()[0] : 0; };

    // ml_upload_table
    std::vector<HostTable> tables(MAX_SLOTS + 1);   // last = centre
    for (int s = 0; s <= MAX_SLOTS; ++s) {
        const std::string p = s == MAX_SLOTS ? "centre." : "table" + std::to_string(s) + ".";
        if (!in.count(p + "values")) continue;
        HostTable &t = tables[s];
        t.h_axis0 = doubles(p + "axis0"), t.h_axis1 = doubles(p + "axis1"), t.h_axis2 = doubles(p + "axis2");
        t.h_order_k = doubles(p + "order_k"), t.h_values = doubles(p + "values");
        t.n0 = (int)t.h_axis0.size(), t.n1 = (int)t.h_axis1.size(), t.n2 = (int)t.h_axis2.size();
        t.n_orders = (int)t.h_order_k.size() / 2;
        if (in[p + "bounds"].count(8) != 6 || t.h_values.size() != (size_t)t.n_orders * t.n0 * t.n1 * t.n2 * 8 ||
            (s == MAX_SLOTS && in[p + "periods"].count(8) != 2))
            return fprintf(stderr, "%s: the arrays of %s do not fit together\n", argv[1], p.c_str()), 2;
        for (int k = 0; k < 6; ++k) t.bounds[k] = in[p + "bounds"].as<double>()[k];
        for (int k = 0; k < 2 && s == MAX_SLOTS; ++k) t.center_periods[k] = in[p + "periods"].as<double>()[k];
        t.present = true;
    }
    const std::vector<double> B = doubles("layout.B"), rc = doubles("layout.r_center"), period = doubles("layout.period"),
                              lateral = doubles("layout.lateral"), cells = doubles("layout.cells");
    const int32_t *ring_gc = in["layout.ring_gc"].as<int32_t>();
    const int n_rings = (int)rc.size(), n_cells = (int)cells.size() / 3;
    if (n_rings < 1 || (int)B.size() != n_rings + 1 || (int)period.size() != n_rings || (int)lateral.size() != n_rings ||
        (int)in["layout.ring_gc"].count(4) != n_rings)
        return fprintf(stderr, "%s: the ring arrays do not fit together\n", argv[1]), 2;
    g_out = fopen(argv[2], "wb");
    if (!g_out) return perror(argv[2]), 2;

    // ml_upload_layout
    const DenseColls D = dense_collections(ring_gc, n_rings);
    if (D.err.code != ML_OK) return fail(argv[2], D.err);
    put("n_colls", D.n_colls);
    put("coll_slot", "i4", D.coll_slot, D.n_colls, 4);
    put("ring_coll", D.ring_coll);
    const RingSearch S = pack_ring_search(B.data(), n_rings);
    if (S.err.code != ML_OK) return fail(argv[2], S.err);
    put("ring_lut", S.lut);
    put("lut_buckets", S.facts.lut_buckets);
    put("lut_inv_h", S.facts.lut_inv_h);
    put("ring_lutrec", "u1", S.rec.data(), S.rec.size() * sizeof(RingBucket), 1);
    put("lutrec_buckets", S.facts.lutrec_buckets);
    put("lutrec_inv_h", S.facts.lutrec_inv_h);
    put("r_outer", S.facts.r_outer);
    put("r_centre", S.facts.r_centre);
    put("n_cells", n_cells);
    if (n_cells > 0) {
        const CellBins C = bin_cells(cells.data(), n_cells);
        if (C.err.code != ML_OK) return fail(argv[2], C.err);
        put("cell_x", C.sx);
        put("cell_y", C.sy);
        put("cell_xy", C.sxy);
        put("cell_which", C.sw);
        put("cell_index", C.si);
        put("slot_of_cell", C.slot_of_cell);
        put("bin_start", C.start);
        put("bins_x", C.facts.bins_x);
        put("bins_y", C.facts.bins_y);
        put("bin_x0", C.facts.x0);
        put("bin_y0", C.facts.y0);
        put("bin_h", C.facts.h);
        const LatticeFit L = fit_lattice(C.sx, C.sy);
        put("lat_ok", (int)L.facts.ok);
        if (L.facts.ok) {
            const std::vector<CellRec> rec = lattice_records(L, C);
            put("cell_lattice_map", L.map);
            put("cell_lattice_rec", "u1", rec.data(), rec.size() * sizeof(CellRec), 1);
            put("lat_c0x", L.facts.c0x);
            put("lat_c0y", L.facts.c0y);
            put("lat_inv", "f8", L.facts.inv, 4, 8);
            put("lat_amin", L.facts.amin);
            put("lat_bmin", L.facts.bmin);
            put("lat_na", L.facts.na);
            put("lat_nb", L.facts.nb);
            put("lat_accept_r2", L.facts.accept_r2);
            put("lat_g", "f8", L.facts.g, 3, 8);
            put("lat_guard", L.facts.guard);
        }
    }

    // the first synthesis: refresh_table_desc, refresh_ring_locations
    std::vector<TableDesc> desc(MAX_SLOTS + 1);
    memset(desc.data(), 0, desc.size() * sizeof(TableDesc));
    for (int s = 0; s <= MAX_SLOTS; ++s)
        if (tables[s].present) desc[s] = describe_table(tables[s], s == MAX_SLOTS);
    put("table_desc", "u1", desc.data(), desc.size() * sizeof(TableDesc), 1);
    const HostTable *slots[MAX_SLOTS], *colls[MAX_RING_COLLS];
    const TableDesc *cdesc[MAX_RING_COLLS];
    for (int s = 0; s < MAX_SLOTS; ++s) slots[s] = &tables[s];
    const RingLocations at = locate_rings(slots, ring_gc, period.data(), n_rings);
    if (at.err.code != ML_OK) return fail(argv[2], at.err);
    for (int c = 0; c < D.n_colls; ++c) {
        colls[c] = slots[D.coll_slot[c]];
        cdesc[c] = &desc[D.coll_slot[c]];
    }
    const LensClass K = classify_lens(colls, D.n_colls, &tables[MAX_SLOTS], knob("force_general") != 0, knob("force_general_coll"));
    put("simple_orders", (int)K.simple);
    put("general_mask", K.general_mask);
    put("centre_general", K.centre_general);
    put("narrow_mask", K.narrow_mask);
    put("wide_mask", K.wide_mask);
    put("narrow_exists", K.narrow_exists);
    put("narrow_slots_max", K.narrow_slots_max);
    const RingInputs rings = {n_rings, D.ring_coll.data(), period.data(), lateral.data(), rc.data()};
    const RingTables T = pack_ring_tables(colls, cdesc, D.coll_slot, D.n_colls, K, rings, at);
    if (T.err.code != ML_OK) return fail(argv[2], T.err);
    put("coll", "u1", T.coll, D.n_colls * sizeof(CollDesc), 1);
    put("ring_bounds_all", "f8", T.ring_bounds_all, 4, 8);
    put("ring_rec", T.rec);
    put("ring_tab", T.tab);
    put("ring_ok", T.ok);
    put("ring_ok_off", T.ok_off);
    CentreTable C;
    if (tables[MAX_SLOTS].present) {
        C = pack_centre_table(tables[MAX_SLOTS], K.centre_simple, K.canon_center);
        put("center_qmajor", C.cq);
    }
    put("center_n_slots", C.slots.n_slots);
    put("center_lo", C.slots.lo);
    put("center_present_mask", C.slots.present);
    return fclose(g_out) ? 1 : 0;
}
