"""NaN-poisoned scratch as pytest fixtures.

Inside facl_amd._lib.poisoned() the partial-sum workspace and every output / scratch tensor the host layer allocates are
filled with NaN bytes before the launches, so a partial row or output element left unwritten at a ragged shape fails the
comparison instead of reading recycled memory.  A graph captured inside it captures the poison fills too, so every replay
starts from NaN scratch.

A module whose every test runs poisoned imports the autouse fixture into its own namespace,

    from poison import poisoned_scratch  # noqa: F401

(an autouse fixture imported into a module applies to that module's tests only); a module that poisons some of its tests
imports `poisoned` and requests it by name."""
import pytest


@pytest.fixture
def poisoned():
    from facl_amd import _lib
    with _lib.poisoned():
        yield


@pytest.fixture(autouse=True)
def poisoned_scratch():
    from facl_amd import _lib
    with _lib.poisoned():
        yield
