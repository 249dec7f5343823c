"""Host side of the element-resolved Rayleigh integral (RayleighAndBHTE.ForwardSteered / ForwardElements,
harness.steering_weights): argument checks that come before any library call, the element layout, and the unit-amplitude
steering weights against the float64 formula. No device is needed."""
import json
import os

import numpy as np
import pytest

from babelbrain_amd import RayleighAndBHTE as R, harness as H

HERE = os.path.dirname(os.path.abspath(__file__))
K = 2 * np.pi * 700e3 / 1500.0


def _geometry(M=12):
    cen = np.arange(3 * M, dtype=np.float32).reshape(M, 3) * 1e-3
    return cen, np.full(M, 1e-6, np.float32), np.array([[0.0, 0.0, 0.1]], np.float32)


def _no_library(monkeypatch):
    def refuse():
        raise AssertionError('the library was loaded before the arguments were checked')
    monkeypatch.setattr(R._engine, 'load_library', refuse)


@pytest.mark.parametrize('elemdims', [5, [4, 4, 3], [[6], [7]], [4, 4, 5]])
def test_counts_must_add_up_to_the_sources(monkeypatch, elemdims):
    _no_library(monkeypatch)
    cen, ds, rf = _geometry(12)
    with pytest.raises(ValueError):
        R.ForwardElements(K, cen, ds, elemdims, rf)
    n = 1 if np.ndim(elemdims) == 0 else len(elemdims)
    with pytest.raises(ValueError):
        R.ForwardSteered(K, cen, ds, elemdims, np.ones((n, 2), np.complex64), rf)


def test_weights_rows_must_match_the_elements(monkeypatch):
    _no_library(monkeypatch)
    cen, ds, rf = _geometry(12)
    for w in (np.ones((2, 3), np.complex64), np.ones(4, np.complex64), np.ones((3, 2, 2), np.complex64)):
        with pytest.raises(ValueError):
            R.ForwardSteered(K, cen, ds, [4, 4, 4], w, rf)
    with pytest.raises(ValueError):
        R.ForwardSteered(K, cen, ds, 4, np.ones((4, 1), np.complex64), rf)        # 12 / 4 = 3 elements


def test_negative_counts_are_refused(monkeypatch):
    _no_library(monkeypatch)
    cen, ds, rf = _geometry(12)
    with pytest.raises(ValueError):
        R.ForwardElements(K, cen, ds, [8, -4, 8], rf)
    with pytest.raises(ValueError):
        R.ForwardSteered(K, cen, ds, [[8], [-4], [8]], np.ones(3, np.complex64), rf)
    with pytest.raises(ValueError):
        R.ForwardElements(K, cen, ds, -4, rf)


def test_elemdims_forms_give_the_same_layout():
    want = np.array([0, 4, 8, 12], np.int64)
    for form in (4, [4, 4, 4], (4, 4, 4), np.array([4, 4, 4]), [[4], [4], [4]], np.array([[4], [4], [4]], np.int32)):
        got = R._elem_start(form, 12)
        assert got.dtype == np.int64 and got.flags.c_contiguous and np.array_equal(got, want), form
    assert np.array_equal(R._elem_start([3, 0, 9], 12), [0, 3, 3, 12])            # an empty element is allowed
    assert np.array_equal(R._elem_start([[3], [0], [9]], 12), [0, 3, 3, 12])
    assert np.array_equal(R._elem_start(12, 12), [0, 12])
    assert np.array_equal(R._elem_start([], 0), [0])


def test_steering_weights_match_the_formula():
    """exp(i angle(conj(p))), p = (i k / 2 pi) exp(-i k R) / R the field of a point source at the focus taken at the element
    centre (CONCAVE:298-314), written out per pair in float64 on the 128 H317 element centres and three foci."""
    ec = np.array(json.load(open(os.path.join(HERE, 'golden', 'h317_elements.json')))['centres_m'], np.float64)
    assert ec.shape == (128, 3)
    foci = np.array([[0.0, 0.0, 135e-3], [10e-3, -5e-3, 125e-3], [-3e-3, 8e-3, 155e-3]])
    for k in (K, complex(K, -4.5)):
        w = H.steering_weights(k, ec, foci)
        kk = complex(k)
        assert w.dtype == np.complex64 and w.shape == (128, 3)
        assert np.abs(np.abs(w.astype(np.complex128)) - 1.0).max() <= 2.0 ** -23
        for e in range(128):
            for s in range(3):
                Rr = float(np.sqrt(((ec[e] - foci[s]) ** 2).sum()))
                p = 1j * kk / (2 * np.pi) * np.exp(-1j * kk * Rr) / Rr
                phi = np.angle(np.conj(p))
                d = np.angle(complex(w[e, s]) * np.exp(-1j * phi))
                assert abs(d) <= 1e-6, (e, s, d)
    one = H.steering_weights(K, ec, foci[1])
    assert one.shape == (128, 1) and np.array_equal(one[:, 0], H.steering_weights(K, ec, foci)[:, 1])


def test_names_of_the_public_interface():
    import inspect
    assert list(inspect.signature(R.ForwardSteered).parameters) == ['cwvnb', 'center', 'ds', 'elemdims', 'weights', 'rf', 'u0', 'deviceMetal']
    assert list(inspect.signature(R.ForwardElements).parameters) == ['cwvnb', 'center', 'ds', 'elemdims', 'rf', 'u0', 'deviceMetal']
    assert 'bfd_rayleigh_forward_elements' in R._engine.ABI_SYMBOLS
