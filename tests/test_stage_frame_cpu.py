"""The frame record of the roll and zoom/crop stages (csrc/planar_layout.h) against what both stages computed per kind of frame
before they walked the plane list: for every format of the table, the planes an entry point builds from its arguments, the analysis
format, and the crop rectangle, result size, source offset and scale factors per plane over a grid of rectangles, odd values and
cw = 1 included (tests/cpp/stage_frame_check.cpp states the old formulas).  Needs no GPU."""
import stage_frame_prog


def test_the_plane_walk_gives_what_the_stages_computed_per_kind():
    rc, out = stage_frame_prog.run()
    assert rc == 0 and out.strip().endswith(" 0 failed"), out[-2000:]
    assert int(out.split()[0]) > 10000
