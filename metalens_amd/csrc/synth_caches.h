// What the synthesis keeps from call to call and when it is dropped: the serials of the three things a synthesis'
// geometry depends on, a stamp per cache (the key it was built for), and the events that drop them, each a member
// function that states what it drops.  DESIGN.md 3.1 holds the table; tests/test_synth_caches.py pins it.
// The callers (ctx.hip, nearfield.hip, farfield.hip, farfield_plan.hip) build a key, ask the stamp, do the work, set the stamp; none of
// them looks inside a key.
//
// Host code without HIP types: compiled by hipcc into the library and by the host compiler into
// tools/synth_caches.cpp, which runs a script of events through it.
#pragma once

namespace ml {

// What a cache was built for: N longs, or nothing.
template <int N>
struct Stamp {
    bool matches(const long (&k)[N]) const {
        if (!valid) return false;
        for (int i = 0; i < N; ++i)
            if (key[i] != k[i]) return false;
        return true;
    }
    void set(const long (&k)[N]) {
        for (int i = 0; i < N; ++i) key[i] = k[i];
        valid = true;
    }
    void forget() { valid = false; }
    bool is_set() const { return valid; }

  private:
    long key[N] = {};
    bool valid = false;
};

// a key, built in place: Key<2> k = {{a, b}}; stamp.matches(k.v)
template <int N>
struct Key {
    long v[N];
};

struct SynthCaches {
    // bumped when the sample axes / the layout / the list of tie answers change
    long grid = 0, layout = 0, overrides = 0;

    Stamp<2> row_extents;   // SynthGrid::row_first (nearfield.hip row_extent_kernel)
    Stamp<2> trim;          // SynthGrid::trim_rows (farfield.hip trim_rows_of)
    Stamp<5> geometry;      // the geometry records and the four patch lists (nearfield_geometry.hip)
    Stamp<6> zeros;         // the zeros outside the lens in the resident field sets
    Stamp<2> answers;       // the (grid, layout) the tie answers were given for; nothing while there are none
    // the lengths of the four patch lists on the host: not known, on their way (queued behind the scans that make
    // them), known
    enum Lengths { UNKNOWN, QUEUED, KNOWN } lengths = UNKNOWN;
    // row_first describes the resident fields: they were synthesised, not uploaded
    bool rows_describe_fields = false;

    // ---- keys ----
    Key<2> grid_layout_key() const { return {{grid, layout}}; }   // row extents, trim rows, tie answers
    // class_word: lens_pack.h list_word - who takes which samples decides which lists exist
    Key<5> geometry_key(long samples, long class_word) const { return {{grid, layout, overrides, samples, class_word}}; }
    Key<6> zeros_key(long buffer, long bytes, long sets, long samples) const {
        return {{buffer, bytes, sets, samples, grid, layout}};
    }

    // ---- events ----
    void grid_changed() { ++grid; }
    void layout_changed() { ++layout; }
    void overrides_changed() { ++overrides; }
    // which patch lists exist and what a synthesis leaves behind depend on who takes which samples
    void lens_class_changed() {
        geometry.forget();
        lengths = UNKNOWN;
        zeros.forget();
    }
    // every patch is visited (and its zeros stored) once more; the lists are new
    void geometry_rebuilt() {
        lengths = UNKNOWN;
        zeros.forget();
    }
    // the caller supplied the fields: nothing is known about zeros, and row_first is not theirs
    void fields_overwritten() {
        zeros.forget();
        rows_describe_fields = false;
    }

    // ---- tie answers ----
    // n answers arrived for the current (grid, layout)
    void answers_given(int n) {
        overrides_changed();
        if (n) {
            answers.set(grid_layout_key().v);
        } else {
            answers.forget();
        }
    }
    // a synthesis begins: answers for another (grid, layout) are dropped.  True: the caller empties its list.
    bool drop_foreign_answers() {
        if (!answers.is_set() || answers.matches(grid_layout_key().v)) return false;
        answers.forget();
        overrides_changed();
        return true;
    }
};

}  // namespace ml
