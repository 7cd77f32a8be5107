"""The synthesis' cache rules (metalens_amd/csrc/synth_caches.h: serials, stamps, events), run on the host by
tools/synth_caches.cpp over scripts of events, against the dependency table of DESIGN.md 3.1 - restated here as
TABLE.  Every script runs through the plain build and through the address / undefined-behaviour sanitizer build of
the tool.  No GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CACHES = ('row_extents', 'trim', 'geometry', 'zeros', 'answers')
SYNTH = 'synth 200 136 1 4096 1740800'
# a context that has synthesised twice and transformed once: every cache fresh, the list lengths on the host
WARM = [SYNTH, 'transform', SYNTH]

# event -> (caches it leaves stale, list lengths afterwards, row_first still describes the fields)
TABLE = {
    'grid': ({'row_extents', 'trim', 'geometry', 'zeros'}, 'known', 1),
    'layout': ({'row_extents', 'trim', 'geometry', 'zeros'}, 'known', 1),
    'overrides': ({'geometry', 'zeros'}, 'known', 1),        # (zeros: a rebuild of the geometry drops them)
    'answers': ({'geometry', 'zeros'}, 'known', 1),          # (they bump the overrides serial)
    'class': ({'geometry', 'zeros'}, 'unknown', 1),
    'rebuilt': ({'zeros'}, 'unknown', 1),
    'upload': ({'zeros'}, 'known', 0),
}


@pytest.fixture(scope='module')
def tool(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('synth_caches')) + os.sep
    subprocess.check_call(['make', '-s', '-j2', '-C', os.path.join(ROOT, 'tools'), 'OUT=' + out, out + 'synth_caches',
                           out + 'synth_caches_san'])

    def run(events):
        """the tool's line per event as a dict (stale: a set), the same from both builds"""
        texts = []
        for exe in ('synth_caches', 'synth_caches_san'):
            res = subprocess.run([out + exe], input='\n'.join(events) + '\n', capture_output=True, text=True, timeout=60)
            assert res.returncode == 0, res.stdout + res.stderr
            texts.append(res.stdout)
        assert texts[0] == texts[1]
        lines = []
        for text in texts[0].splitlines():
            event, *facts = text.split()
            d = dict(kv.split('=') for kv in facts)
            d['stale'] = set() if d['stale'] == '-' else set(d['stale'].split(','))
            assert d['stale'] <= set(CACHES)
            lines.append(dict(d, event=event))
        assert [ln['event'] for ln in lines] == [e.split()[0] for e in events]
        return lines
    return run


def serials(line):
    return tuple(int(line[k]) for k in ('grid', 'layout', 'overrides'))


def test_first_synthesis_builds_everything_and_a_repeat_finds_all_fresh(tool):
    first, trim, second, third = tool(WARM + [SYNTH])
    assert first['stale'] == {'row_extents', 'trim', 'geometry', 'zeros'} and first['lengths'] == 'queued'
    assert trim['stale'] == set()
    # the second synthesis finds the zeros stored and fetches the queued list lengths; the third finds them there
    assert second['stale'] == set() and second['lengths'] == 'known' and second['rows'] == '1'
    assert third['stale'] == set() and third['lengths'] == 'known'
    assert serials(first) == serials(third) == (0, 0, 0)


@pytest.mark.parametrize('event', sorted(TABLE))
def test_every_event_drops_exactly_what_the_table_says(tool, event):
    stale, lengths, rows = TABLE[event]
    lines = tool(WARM + [event, SYNTH, 'transform', SYNTH])
    before, after, again = lines[2], lines[3], lines[4]
    assert after['stale'] == stale and after['lengths'] == lengths and int(after['rows']) == rows
    bumped = {'grid': 0, 'layout': 1, 'overrides': 2, 'answers': 2}.get(event)
    want = list(serials(before))
    if bumped is not None:
        want[bumped] += 1
    assert serials(after) == tuple(want)
    # the next synthesis finds exactly that stale, rebuilds it, and the one after finds all fresh again
    assert again['stale'] == stale and again['rows'] == '1' and again['dropped'] == '0'
    assert again['lengths'] == ('queued' if 'geometry' in stale else lengths)
    assert lines[6]['stale'] == set() and lines[6]['lengths'] == 'known'


@pytest.mark.parametrize('changed', ['synth 200 136 2 4096 1740800',      # set count
                                     'synth 200 136 1 8192 1740800',      # buffer address
                                     'synth 200 136 1 4096 3481600'])     # byte size
def test_sets_buffer_and_bytes_each_stale_the_zeros_alone(tool, changed):
    lines = tool(WARM + [changed, changed, SYNTH])
    assert lines[3]['stale'] == {'zeros'} and lines[3]['lengths'] == 'known'
    assert lines[4]['stale'] == set()
    assert lines[5]['stale'] == {'zeros'}        # (one stamp: the zeros are known for the last writer only)
    assert serials(lines[5]) == (0, 0, 0)


def test_another_sample_count_rebuilds_geometry_and_zeros(tool):
    lines = tool(WARM + ['synth 100 136 1 4096 1740800'])
    assert lines[3]['stale'] == {'geometry', 'zeros'} and lines[3]['lengths'] == 'queued'


def test_answers_for_another_grid_or_layout_are_dropped_by_the_next_synthesis(tool):
    for moved in ('grid', 'layout'):
        lines = tool(WARM + ['answers', SYNTH, SYNTH, moved, SYNTH, SYNTH, SYNTH])
        given, with_answers, kept, event, dropping, after, fresh = lines[3:]
        assert serials(given)[2] == 1 and with_answers['stale'] == {'geometry', 'zeros'}
        # a synthesis on the same (grid, layout) keeps them
        assert kept['stale'] == set() and kept['dropped'] == '0' and serials(kept)[2] == 1
        assert 'answers' in event['stale'] and serials(event)[2] == 1
        # the drop bumps the overrides serial, and so (besides the moved serial) rebuilds the geometry
        assert dropping['dropped'] == '1' and serials(dropping)[2] == 2
        assert dropping['stale'] == {'row_extents', 'trim', 'geometry', 'zeros', 'answers'}
        assert after['dropped'] == '0' and after['stale'] == {'trim'} and serials(after)[2] == 2
        assert fresh['stale'] == {'trim'} and fresh['lengths'] == 'known'


def test_an_empty_answer_list_is_never_dropped(tool):
    lines = tool(WARM + ['answers 0', SYNTH, 'grid', SYNTH])
    assert serials(lines[3])[2] == 1 and lines[4]['stale'] == {'geometry', 'zeros'}
    assert 'answers' not in lines[5]['stale']
    assert lines[6]['dropped'] == '0' and serials(lines[6])[2] == 1


def test_uploaded_fields_have_no_trim_until_the_next_synthesis(tool):
    lines = tool(WARM + ['grid', 'upload', 'transform', SYNTH, 'transform'])
    assert lines[5]['stale'] == {'row_extents', 'trim', 'geometry', 'zeros'} and lines[5]['rows'] == '0'   # not built
    assert lines[6]['rows'] == '1' and lines[7]['stale'] == set()
