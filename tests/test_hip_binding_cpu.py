"""CPU: `_hip.parse_header` turns C declarations in the format of include/salience_hip.h into ctypes signatures and
struct fields, refuses what it does not know, and `_hip.launch` only takes entry points that enqueue on a stream."""
import ctypes

import pytest

from salience_detr_amd import _hip

P, I, I64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64

HEADER = """
/* a comment with a declaration inside: int sdetr_not_this(int a); */
#ifndef EXAMPLE_H_
#define EXAMPLE_VERSION 1
typedef struct ihipStream_t *sdetr_stream_t; /* == hipStream_t */
const char *sdetr_last_error(void);
size_t sdetr_scratch_bytes(int batch_size, int64_t rows);
typedef struct {
    const float *a, *b; /* two pointers in one declaration */
    int64_t n;
    int batch, rows;
} sdetr_pair_job;
int sdetr_resize(sdetr_stream_t stream, const void *const *images, const int *image_hw /* host */, int64_t total,
                 float scale, double eps, const sdetr_pair_job *job, const int32_t level_hw[8], size_t workspace_bytes,
                 float *out);
#endif
"""


def test_parser_gives_exact_ctypes():
    signatures, structs, launches = _hip.parse_header(HEADER)
    assert signatures == {
        "sdetr_last_error": (ctypes.c_char_p, []),
        "sdetr_scratch_bytes": (ctypes.c_size_t, [I, I64]),
        "sdetr_resize": (I, [P, P, P, I64, ctypes.c_float, ctypes.c_double, P, P, ctypes.c_size_t, P]),
    }
    assert structs == {"sdetr_pair_job": [("a", P), ("b", P), ("n", I64), ("batch", I), ("rows", I)]}
    assert launches == {"sdetr_resize"}


@pytest.mark.parametrize("declaration", [
    "int sdetr_f(sdetr_stream_t stream, unsigned n);",            # a type the table does not hold
    "uint8_t sdetr_f(void);",                                     # ... as a return type
    "int sdetr_f(int);",                                          # a parameter without a name
    "typedef struct { uint8_t flag; } sdetr_s;",                  # ... as a struct field
    "int other_f(int a);",                                        # not an sdetr_ function
    "int sdetr_f(int a)",                                         # no semicolon
])
def test_parser_refuses_what_it_does_not_know(declaration):
    with pytest.raises(_hip.HipExtensionError):
        _hip.parse_header(declaration)


def test_unknown_type_error_names_the_declaration():
    with pytest.raises(_hip.HipExtensionError, match="unsigned n.*sdetr_f"):
        _hip.parse_header("int sdetr_f(sdetr_stream_t stream, unsigned n);")


def test_real_header_knows_which_entry_points_are_launches():
    assert "sdetr_ffn_auto_splits" in _hip.SIGNATURES and "sdetr_ffn_auto_splits" not in _hip.LAUNCHES
    assert "sdetr_gather_rows" in _hip.LAUNCHES and _hip.LAUNCHES <= set(_hip.SIGNATURES)
    assert all(_hip.SIGNATURES[name][1][0] is P for name in _hip.LAUNCHES)


def test_launch_refuses_an_entry_point_without_a_stream(monkeypatch):
    """``sdetr_ffn_auto_splits(tokens, hidden)`` takes no stream: ``launch`` raises before it loads or calls anything."""
    def no_call(*a, **k):
        raise AssertionError("launch went on to the library")
    monkeypatch.setattr(_hip, "lib", no_call)
    with pytest.raises(_hip.HipExtensionError, match="sdetr_ffn_auto_splits is not a launch"):
        _hip.launch("sdetr_ffn_auto_splits", None, "cuda:0", 1800, 2048)
