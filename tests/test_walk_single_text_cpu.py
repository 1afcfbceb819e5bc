"""The catalogue walk has one text: the blocks that k_recommend, k_rank_count, k_priced, k_quota,
k_group and k_explore have in common are the csrc/walk_*.inc fragments, included at the point of use.  This guard reads
files only: every fragment holds its sentinel line, no file that includes a fragment also writes that line out, and
the files include exactly the fragments the table of section 31 lists for them."""
import glob
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "collaborative-filtering_amd", "csrc")

# one line of each fragment that a written-out copy of its block could not do without
SENTINELS = {
    "walk_seen_cursor.inc": "if (seen_idx[mid] < lo) a = mid + 1; else e = mid;",
    "walk_seen_masks.inc": "bool near = false;",
    "walk_z_fetch.inc": "pf[p] = *reinterpret_cast<const f32x4*>(Z + (size_t)min(it0 + i, n - 1) * ld + 4 * d);",
    "walk_z_stage.inc": "*reinterpret_cast<f32x4*>(&zs[i][4 * d]) = pf[p];",
    "walk_allow_scan.inc": "auto next_chunk = [&]",
    "walk_score_tiles.inc": "acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(ua[e], z1[e], acc1, 0, 0, 0);",
    "walk_row_lists.inc": "auto compact = [&](int r) {",
    "walk_row_overflow.inc": "if (rc > BUF - walk::CHUNK) compact(r);",
    "walk_row_write.inc": "if (lane == 0) top_cnt[rb] = rn;",
}
WALKERS = ("recommend.hip", "rank_eval.hip", "capacity.hip", "quota.hip")


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _design_table():
    """{fragment: set of the .hip files that section 31 says include it}, from the rows `| `walk_x.inc` | block | files |`."""
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        section = f.read().split("\n## 31.", 1)[1].split("\n## ", 1)[0]
    rows = {}
    for line in section.splitlines():
        m = re.match(r"\| `(walk_\w+\.inc)` \|[^|]*\| ([^|]*) \|", line)
        if m:
            rows[m.group(1)] = {name.strip() + ".hip" for name in m.group(2).split(",")}
    return rows


def _includers(fragment):
    pattern = re.compile(r'^#include "%s"$' % re.escape(fragment), re.M)
    names = [os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*.hip"))]
    return {name for name in names if pattern.search(_read(name))}


def test_section_31_lists_the_fragments_that_exist():
    on_disk = {os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*.inc"))}
    assert on_disk == set(SENTINELS) == set(_design_table())


@pytest.mark.parametrize("fragment", sorted(SENTINELS))
def test_a_fragment_is_the_only_text_of_its_block(fragment):
    sentinel = SENTINELS[fragment]
    assert _read(fragment).count(sentinel) == 1
    includers = _includers(fragment)
    assert includers == _design_table()[fragment]
    for name in sorted(includers):
        text = _read(name)
        assert sentinel not in text, f"{name} includes {fragment} and writes its block out as well"
        assert text.count(f'#include "{fragment}"') == 1


@pytest.mark.parametrize("name", WALKERS)
def test_the_four_walkers_include_what_section_31_lists_for_them(name):
    listed = {fragment for fragment, files in _design_table().items() if name in files}
    assert len(listed) >= 6                               # cursor, masks, fetch, stage, scan, tiles at the least
    text = _read(name)
    for fragment in sorted(listed):
        assert f'#include "{fragment}"' in text


def test_a_fragment_is_plain_statements():
    for fragment in SENTINELS:
        code = [line for line in _read(fragment).splitlines() if not line.lstrip().startswith("//")]
        directives = {line.split()[0] + " " + line.split()[1] for line in code if line.startswith("#")}
        assert directives <= {"#pragma unroll"}, (fragment, directives)      # no #define, no #if, no nested #include
        assert _read(fragment).startswith("// Catalogue walk,") and "expects" in _read(fragment)
