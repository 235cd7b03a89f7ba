"""The float INTER_AREA (csrc/dyn_ingest.h: k_resize_area_f32) and the batched virtual views (csrc/dyn_splat.h: dyn_vv_frames) under the
wave-level emulator: the checks of tests/test_gpu_vv_ingest.py through vv_ingest_cases, without the end-to-end scene and the tool.
Debugging aid in a container without a GPU; -m gpu is authoritative."""
import pytest

import vv_ingest_cases as vc

pytestmark = pytest.mark.emu


@pytest.mark.parametrize('C', [1, 3])
@pytest.mark.parametrize('Hs,Ws,Hd,Wd', vc.AREA_F32_CASES)
def test_resize_area_f32(emu, Hs, Ws, Hd, Wd, C):
  vc.check_area_f32(emu, Hs, Ws, Hd, Wd, C)


def test_resize_area_f32_into_a_pitched_store(emu):
  vc.check_area_f32_pitched(emu)


def test_resize_area_f32_refusals(emu):
  vc.check_area_f32_refusals(emu)


def test_virtual_views_equal_the_per_frame_path(emu):
  vc.check_views_equal_the_per_frame_path(emu)


def test_virtual_views_with_per_frame_intrinsics_that_differ(emu):
  vc.check_per_frame_intrinsics_that_differ(emu)


def test_virtual_views_in_more_than_one_sort_group(emu):
  vc.check_more_than_one_sort_group(emu)


def test_virtual_views_one_frame_one_view(emu):
  vc.check_one_frame_one_view(emu)


def test_virtual_views_with_points_behind_the_camera(emu):
  vc.check_points_behind_the_camera(emu)


def test_virtual_views_refusals(emu):
  vc.check_views_refusals(emu)
