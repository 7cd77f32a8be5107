// Runs a script of events through the synthesis' cache rules (metalens_amd/csrc/synth_caches.h) in the order the
// library meets them, and prints after each event which caches are stale.  Runs without a GPU.
//
//   synth_caches SCRIPT        (or the script on standard input)
//
// One event per line ('#' starts a comment):
//   grid | layout | overrides        the sample axes / the layout / the list of tie answers changed (the serials)
//   class [WORD]                     the lens class changed (ctx.hip refresh_ring_locations); WORD: the new word of the
//                                    geometry key (lens_pack.h LensClass::list_word), else it stays
//   rebuilt                          the geometry records were rebuilt (nearfield.hip ensure_geometry)
//   upload                           ml_fields_upload
//   answers [N]                      ml_nearfield_tie_answers with N answers (default 1)
//   synth NX NY SETS BUFFER BYTES    a synthesis (ctx.hip nearfield_prepare, nearfield.hip nearfield_launch) of SETS
//                                    field sets of NX x NY samples into the buffer at BUFFER of BYTES bytes
//   transform                        a far-field transform's row trim (farfield.hip trim_rows_of)
// Output, one line per event:
//   EVENT stale=<comma list or -> grid=G layout=L overrides=O lengths=unknown|queued|known rows=0|1 dropped=0|1
// stale: of row_extents, trim, geometry, zeros, answers - after `synth` what that synthesis FOUND stale (and rebuilt;
// trim as it stands: a synthesis does not consult it), after any other event what a synthesis with the arguments of
// the last one (and a transform) would find.  answers is stale when answers are held for another (grid, layout).
// dropped: that synthesis dropped such answers.  rows: row_first describes the resident fields.
// Build + run:  make -C tools synth_caches && printf 'synth 8 8 1 4096 4096\ngrid\n' | tools/synth_caches
#include <cstdio>
#include <cstring>
#include <string>

#include "synth_caches.h"

using namespace ml;

struct Shape {
    long nx = 0, ny = 0, sets = 1, buffer = 0, bytes = 0, word = -2;
};

struct Stale {
    bool row_extents, trim, geometry, zeros, answers;
};

static Stale stale_now(const SynthCaches &c, const Shape &s) {
    const Key<2> gl = c.grid_layout_key();
    const bool geometry = !c.geometry.matches(c.geometry_key(s.nx * s.ny, s.word).v);
    // (a rebuild of the geometry drops the zeros: SynthCaches::geometry_rebuilt)
    return {!c.row_extents.matches(gl.v), !c.trim.matches(gl.v), geometry,
            geometry || !c.zeros.matches(c.zeros_key(s.buffer, s.bytes, s.sets, s.nx * s.ny).v),
            c.answers.is_set() && !c.answers.matches(gl.v)};
}

// nearfield_prepare and nearfield_launch, the cache rules alone, in their order
static Stale synthesise(SynthCaches &c, const Shape &s, bool *dropped) {
    Stale found = stale_now(c, s);
    *dropped = c.drop_foreign_answers();
    c.rows_describe_fields = true;
    const Key<2> gl = c.grid_layout_key();
    if (found.row_extents) c.row_extents.set(gl.v);
    const Key<5> geo = c.geometry_key(s.nx * s.ny, s.word);
    found.geometry = !c.geometry.matches(geo.v);
    if (found.geometry) {
        c.geometry.set(geo.v);
        c.geometry_rebuilt();
        c.lengths = SynthCaches::QUEUED;
    }
    const Key<6> zeros = c.zeros_key(s.buffer, s.bytes, s.sets, s.nx * s.ny);
    found.zeros = !c.zeros.matches(zeros.v);
    if (!found.zeros) c.lengths = SynthCaches::KNOWN;
    c.zeros.set(zeros.v);
    return found;
}

int main(int argc, char **argv) {
    FILE *in = argc > 1 ? fopen(argv[1], "r") : stdin;
    if (!in) return perror(argv[1]), 2;
    SynthCaches c;
    Shape shape;
    char line[256];
    while (fgets(line, sizeof line, in)) {
        if (char *hash = strchr(line, '#')) *hash = 0;
        char ev[32];
        long v[5] = {0, 0, 0, 0, 0};
        const int got = sscanf(line, "%31s %ld %ld %ld %ld %ld", ev, &v[0], &v[1], &v[2], &v[3], &v[4]);
        if (got < 1) continue;
        const std::string e = ev;
        bool dropped = false, is_synth = false;
        Stale st;
        if (e == "grid") c.grid_changed();
        else if (e == "layout") c.layout_changed();
        else if (e == "overrides") c.overrides_changed();
        else if (e == "class") {
            c.lens_class_changed();
            if (got >= 2) shape.word = v[0];
        } else if (e == "rebuilt") c.geometry_rebuilt();
        else if (e == "upload") c.fields_overwritten();
        else if (e == "answers") c.answers_given(got >= 2 ? (int)v[0] : 1);
        else if (e == "transform") {
            if (c.rows_describe_fields && !c.trim.matches(c.grid_layout_key().v)) c.trim.set(c.grid_layout_key().v);
        } else if (e == "synth" && got == 6) {
            shape.nx = v[0], shape.ny = v[1], shape.sets = v[2], shape.buffer = v[3], shape.bytes = v[4];
            st = synthesise(c, shape, &dropped);
            is_synth = true;
        } else
            return fprintf(stderr, "bad event: %s", line), 2;
        if (!is_synth) st = stale_now(c, shape);
        std::string list;
        const char *names[5] = {"row_extents", "trim", "geometry", "zeros", "answers"};
        const bool flags[5] = {st.row_extents, st.trim, st.geometry, st.zeros, st.answers};
        for (int k = 0; k < 5; ++k)
            if (flags[k]) list += (list.empty() ? "" : ",") + std::string(names[k]);
        const char *lengths[3] = {"unknown", "queued", "known"};
        printf("%s stale=%s grid=%ld layout=%ld overrides=%ld lengths=%s rows=%d dropped=%d\n", ev,
               list.empty() ? "-" : list.c_str(), c.grid, c.layout, c.overrides, lengths[c.lengths],
               (int)c.rows_describe_fields, (int)dropped);
    }
    return 0;
}
