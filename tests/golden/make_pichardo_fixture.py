#!/usr/bin/env python3
"""Cuts tests/golden/pichardo_excerpt.h5 out of the reference's TranscranialModeling/MapPichardo.h5.

The excerpt keeps what the real H5pySimple wrote, byte for byte: `rho` and `freq` are copied whole (H5Ocopy keeps the
Blosc-compressed chunks and the `type` attribute as they are), and of the two 500 x 500 maps `MapSoS` and `MapAtt` the
first stored chunk is moved over raw (H5Dread_chunk / H5Dwrite_chunk: never decompressed or compressed again) into a
dataset of one chunk with the original's creation properties. Reading the excerpt therefore exercises the same Blosc
decoding as reading the original, at a few tens of KB instead of 2.5 MB.
Usage: python tests/golden/make_pichardo_fixture.py <reference tree>/TranscranialModeling/MapPichardo.h5
"""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from babelbrain_amd import datafile as DF  # noqa: E402

DST = os.path.join(HERE, 'pichardo_excerpt.h5')


def main(src_path):
    L = DF._h5()
    hid, hsize = ctypes.c_int64, ctypes.c_uint64
    for name, res, args in (('H5Ocopy', ctypes.c_int, [hid, ctypes.c_char_p, hid, ctypes.c_char_p, hid, hid]),
                            ('H5Dget_create_plist', hid, [hid]),
                            ('H5Pget_chunk', ctypes.c_int, [hid, ctypes.c_int, ctypes.c_void_p]),
                            ('H5Pclose', ctypes.c_int, [hid]),
                            ('H5Dget_chunk_storage_size', ctypes.c_int, [hid, ctypes.c_void_p, ctypes.POINTER(hsize)]),
                            ('H5Dread_chunk', ctypes.c_int, [hid, hid, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32), ctypes.c_void_p]),
                            ('H5Dwrite_chunk', ctypes.c_int, [hid, hid, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p])):
        f = getattr(L, name)
        f.restype, f.argtypes = res, args
    ck = DF._ck
    src = ck(L.H5Fopen(src_path.encode(), 0, 0), 'H5Fopen')            # H5F_ACC_RDONLY
    dst = ck(L.H5Fcreate(DST.encode(), 2, 0, 0), 'H5Fcreate')          # H5F_ACC_TRUNC
    for name in (b'rho', b'freq'):
        ck(L.H5Ocopy(src, name, dst, name, 0, 0), 'H5Ocopy')
    # H5Dcreate2 refuses a pipeline whose filter cannot encode; the chunks below are written raw, so a stand-in Blosc class
    # that claims an encoder and fails every call is enough (it replaces the decode-only one in this process only)
    FILTER = ctypes.CFUNCTYPE(ctypes.c_size_t, ctypes.c_uint, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t,
                              ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_void_p))

    class H5ZClass(ctypes.Structure):
        _fields_ = [('version', ctypes.c_int), ('id', ctypes.c_int), ('encoder_present', ctypes.c_uint),
                    ('decoder_present', ctypes.c_uint), ('name', ctypes.c_char_p), ('can_apply', ctypes.c_void_p),
                    ('set_local', ctypes.c_void_p), ('filter', FILTER)]
    refuse = FILTER(lambda *a: 0)
    stand_in = H5ZClass(1, DF._BLOSC_ID, 1, 1, b'blosc stand-in (raw chunk writes only)', None, None, refuse)
    ck(L.H5Zregister(ctypes.byref(stand_in)), 'H5Zregister')
    for name in (b'MapSoS', b'MapAtt'):
        d = ck(L.H5Dopen2(src, name, 0), 'H5Dopen2')
        dcpl = ck(L.H5Dget_create_plist(d), 'H5Dget_create_plist')
        chunk = np.zeros(2, np.uint64)
        if L.H5Pget_chunk(dcpl, 2, chunk.ctypes.data) != 2:
            raise RuntimeError('%s is not a chunked 2-D dataset' % name)
        off = np.zeros(2, np.uint64)
        nbytes = hsize()
        ck(L.H5Dget_chunk_storage_size(d, off.ctypes.data, ctypes.byref(nbytes)), 'H5Dget_chunk_storage_size')
        raw = ctypes.create_string_buffer(nbytes.value)
        filt = ctypes.c_uint32()
        ck(L.H5Dread_chunk(d, 0, off.ctypes.data, ctypes.byref(filt), raw), 'H5Dread_chunk')
        ftype = ck(L.H5Dget_type(d), 'H5Dget_type')
        space = ck(L.H5Screate_simple(2, chunk.ctypes.data, None), 'H5Screate_simple')
        out = ck(L.H5Dcreate2(dst, name, ftype, space, 0, dcpl, 0), 'H5Dcreate2')
        ck(L.H5Dwrite_chunk(out, 0, filt.value, off.ctypes.data, nbytes.value, raw), 'H5Dwrite_chunk')
        DF._set_type_attr(out, 'ndarray')
        for h, close in ((out, L.H5Dclose), (space, L.H5Sclose), (ftype, L.H5Tclose), (dcpl, L.H5Pclose), (d, L.H5Dclose)):
            close(h)
    L.H5Fclose(dst)
    L.H5Fclose(src)
    print('%s: %d bytes' % (DST, os.path.getsize(DST)))


if __name__ == '__main__':
    main(sys.argv[1])
