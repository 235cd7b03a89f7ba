"""dynibar_amd.engine.select off the GPU: what it refuses before any library is bound."""
import os

import pytest

from dynibar_amd import _lib, engine


@pytest.fixture
def unbound(monkeypatch):
  monkeypatch.setattr(_lib, '_LIB', None)
  monkeypatch.setattr(_lib, 'LIB_PATH', _lib.LIB_PATH)
  monkeypatch.delenv('DYNIBAR_HIP_LIB', raising=False)
  return monkeypatch


def test_unknown_name_is_a_value_error(unbound):
  with pytest.raises(ValueError, match="'fast'"):
    engine.select('fast')


def test_an_explicit_library_path_is_not_overridden(unbound):
  unbound.setenv('DYNIBAR_HIP_LIB', '/somewhere/else/libdynibar_hip_dev.so')
  before = _lib.LIB_PATH
  with pytest.raises(RuntimeError, match='DYNIBAR_HIP_LIB'):
    engine.select('half')
  assert _lib.LIB_PATH == before
  unbound.setenv('DYNIBAR_HIP_LIB', _lib.engine_path('half'))
  engine.select('half')  # the same file: no conflict, nothing changes
  assert _lib.LIB_PATH == before


def test_a_flavour_that_is_not_built_is_an_error_not_another_engine(unbound):
  unbound.setattr(_lib, 'ENGINE_LIBS', dict(_lib.ENGINE_LIBS, half='libdynibar_hip_not_built.so'))
  before = _lib.LIB_PATH
  with pytest.raises(RuntimeError, match='libdynibar_hip_not_built.so is missing'):
    engine.select('half')
  assert _lib.LIB_PATH == before


def test_select_names_the_bound_library_when_it_is_too_late(unbound):
  class Bound:
    _name = '/x/libdynibar_hip_x1.so'
  unbound.setattr(_lib, '_LIB', Bound())
  assert _lib.bound_path() == '/x/libdynibar_hip_x1.so'
  with pytest.raises(RuntimeError, match='libdynibar_hip_x1.so is already loaded'):
    engine.select('split')
