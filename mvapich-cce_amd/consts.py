"""Handle values of the reference ABI (include/mpi.h:64-140, mpi_errno.h:24-49).

Mirrors include/mvx_mpi.h; numpy dtypes give the element layout of each
datatype on x86-64 (the reference's C types; pair structs per initdte.c:74-104).
"""
import numpy as np

MPI_PACKED, MPI_LB, MPI_UB = 14, 15, 16
MPI_CHAR, MPI_UNSIGNED_CHAR, MPI_BYTE, MPI_SHORT, MPI_UNSIGNED_SHORT = 1, 2, 3, 4, 5
MPI_INT, MPI_UNSIGNED, MPI_LONG, MPI_UNSIGNED_LONG = 6, 7, 8, 9
MPI_FLOAT, MPI_DOUBLE, MPI_LONG_DOUBLE, MPI_LONG_LONG_INT = 10, 11, 12, 13
MPI_LONG_LONG = 13
MPI_FLOAT_INT, MPI_DOUBLE_INT, MPI_LONG_INT, MPI_SHORT_INT, MPI_2INT, MPI_LONG_DOUBLE_INT = 17, 18, 19, 20, 21, 22
MPI_COMPLEX, MPI_DOUBLE_COMPLEX = 23, 24
# the Fortran types of a Fortran-enabled build (mpi.h:104-113, initfutil.c:220-349)
MPI_LOGICAL, MPI_REAL, MPI_DOUBLE_PRECISION, MPI_INTEGER = 25, 26, 27, 28
MPI_2INTEGER, MPI_2COMPLEX, MPI_2DOUBLE_COMPLEX, MPI_2REAL, MPI_2DOUBLE_PRECISION = 29, 30, 31, 32, 33
MPI_CHARACTER = 1
MPI_UNSIGNED_LONG_LONG = 35
# EXTENSION beyond the reference ABI (include/mvx_mpi.h): the 16-bit floats
MVX_FLOAT16, MVX_BFLOAT16 = 64, 65
# and the 8-bit OCP floats (e4m3fn, e5m2)
MVX_FLOAT8_E4M3, MVX_FLOAT8_E5M2 = 72, 73

MPI_OP_NULL = 0
MPI_MAX, MPI_MIN, MPI_SUM, MPI_PROD, MPI_LAND, MPI_BAND = 100, 101, 102, 103, 104, 105
MPI_LOR, MPI_BOR, MPI_LXOR, MPI_BXOR, MPI_MINLOC, MPI_MAXLOC = 106, 107, 108, 109, 110, 111
# EXTENSION (include/mvx_mpi.h): SUM / PROD accumulated in f32 and narrowed once
MVX_SUM_ACC32, MVX_PROD_ACC32 = 164, 165
F32_OUT, F32_IN = 1, 2                       # mvx_op_program_f32's side (include/mvx_hip.h)

MPI_COMM_WORLD, MPI_COMM_SELF = 91, 92

MPI_SUCCESS, MPI_ERR_BUFFER, MPI_ERR_COUNT, MPI_ERR_TYPE = 0, 1, 2, 3
MPI_ERR_COMM, MPI_ERR_ROOT, MPI_ERR_OP, MPI_ERR_ARG, MPI_ERR_OTHER, MPI_ERR_INTERN = 5, 7, 9, 12, 15, 16
ERR_OP_NOT_DEFINED = 329   # MPIR_ERRCLASS_TO_CODE(MPI_ERR_OP, MPIR_ERR_NOT_DEFINED)

SHAPE_TREE, SHAPE_CHAIN = 0, 1
COLL_ALLREDUCE, COLL_REDUCE, COLL_REDUCE_SCATTER, COLL_SCAN = 1, 2, 3, 4
ALG_NONE, ALG_RECDBL, ALG_RABENSEIFNER, ALG_BINOMIAL, ALG_RS_HALVING, ALG_RS_PAIRWISE, ALG_SCAN_RECDBL, \
    ALG_RS_RECDBL, ALG_SMP_LEADER = range(9)
OPKIND_PREDEFINED, OPKIND_USER_COMMUTE, OPKIND_USER_NONCOMMUTE = 0, 1, 2
EXCH_P2P, EXCH_PIPE, EXCH_COLL = 0, 1, 2     # mvx_comm_set_exchange (include/mvx_coll.h)

PAIR_FLOAT_INT = np.dtype([("v", np.float32), ("l", np.int32)])
PAIR_DOUBLE_INT = np.dtype({"names": ["v", "l"], "formats": [np.float64, np.int32], "offsets": [0, 8], "itemsize": 16})
PAIR_LONG_INT = np.dtype({"names": ["v", "l"], "formats": [np.int64, np.int32], "offsets": [0, 8], "itemsize": 16})
PAIR_SHORT_INT = np.dtype({"names": ["v", "l"], "formats": [np.int16, np.int32], "offsets": [0, 4], "itemsize": 8})
PAIR_2INT = np.dtype([("v", np.int32), ("l", np.int32)])
# contiguous(2, x): value and loc both of type x
PAIR_2REAL = np.dtype([("v", np.float32), ("l", np.float32)])
PAIR_2DOUBLE = np.dtype([("v", np.float64), ("l", np.float64)])
PAIR_2COMPLEX = np.dtype([("v", np.complex64), ("l", np.complex64)])
PAIR_2DCOMPLEX = np.dtype([("v", np.complex128), ("l", np.complex128)])
# x87 80-bit long double in a 16-byte slot (x86-64 numpy longdouble)
PAIR_LONG_DOUBLE_INT = np.dtype({"names": ["v", "l"], "formats": [np.longdouble, np.int32], "offsets": [0, 16],
                                 "itemsize": 32})

NP_DTYPE = {
    MPI_CHAR: np.dtype(np.int8), MPI_UNSIGNED_CHAR: np.dtype(np.uint8), MPI_BYTE: np.dtype(np.uint8),
    MPI_SHORT: np.dtype(np.int16), MPI_UNSIGNED_SHORT: np.dtype(np.uint16),
    MPI_INT: np.dtype(np.int32), MPI_UNSIGNED: np.dtype(np.uint32),
    MPI_LONG: np.dtype(np.int64), MPI_UNSIGNED_LONG: np.dtype(np.uint64), MPI_LONG_LONG_INT: np.dtype(np.int64),
    MPI_FLOAT: np.dtype(np.float32), MPI_DOUBLE: np.dtype(np.float64),
    MPI_COMPLEX: np.dtype(np.complex64), MPI_DOUBLE_COMPLEX: np.dtype(np.complex128),
    MPI_FLOAT_INT: PAIR_FLOAT_INT, MPI_DOUBLE_INT: PAIR_DOUBLE_INT, MPI_LONG_INT: PAIR_LONG_INT,
    MPI_SHORT_INT: PAIR_SHORT_INT, MPI_2INT: PAIR_2INT,
    MPI_LONG_DOUBLE: np.dtype(np.longdouble), MPI_LONG_DOUBLE_INT: PAIR_LONG_DOUBLE_INT,
    MPI_LOGICAL: np.dtype(np.int32), MPI_REAL: np.dtype(np.float32), MPI_DOUBLE_PRECISION: np.dtype(np.float64),
    MPI_INTEGER: np.dtype(np.int32), MPI_2INTEGER: PAIR_2INT, MPI_2REAL: PAIR_2REAL,
    MPI_2DOUBLE_PRECISION: PAIR_2DOUBLE, MPI_2COMPLEX: PAIR_2COMPLEX, MPI_2DOUBLE_COMPLEX: PAIR_2DCOMPLEX,
    # numpy has no bfloat16: its elements are uint16 bit patterns
    MVX_FLOAT16: np.dtype(np.float16), MVX_BFLOAT16: np.dtype(np.uint16),
    # nor the 8-bit floats: uint8 bit patterns
    MVX_FLOAT8_E4M3: np.dtype(np.uint8), MVX_FLOAT8_E5M2: np.dtype(np.uint8),
}

OP_NAMES = {MPI_MAX: "MPI_MAX", MPI_MIN: "MPI_MIN", MPI_SUM: "MPI_SUM", MPI_PROD: "MPI_PROD",
            MPI_LAND: "MPI_LAND", MPI_BAND: "MPI_BAND", MPI_LOR: "MPI_LOR", MPI_BOR: "MPI_BOR",
            MPI_LXOR: "MPI_LXOR", MPI_BXOR: "MPI_BXOR", MPI_MINLOC: "MPI_MINLOC", MPI_MAXLOC: "MPI_MAXLOC",
            MVX_SUM_ACC32: "MVX_SUM_ACC32", MVX_PROD_ACC32: "MVX_PROD_ACC32"}
TYPE_NAMES = {MPI_CHAR: "MPI_CHAR", MPI_UNSIGNED_CHAR: "MPI_UNSIGNED_CHAR", MPI_BYTE: "MPI_BYTE",
              MPI_SHORT: "MPI_SHORT", MPI_UNSIGNED_SHORT: "MPI_UNSIGNED_SHORT", MPI_INT: "MPI_INT",
              MPI_UNSIGNED: "MPI_UNSIGNED", MPI_LONG: "MPI_LONG", MPI_UNSIGNED_LONG: "MPI_UNSIGNED_LONG",
              MPI_FLOAT: "MPI_FLOAT", MPI_DOUBLE: "MPI_DOUBLE", MPI_LONG_DOUBLE: "MPI_LONG_DOUBLE",
              MPI_LONG_LONG_INT: "MPI_LONG_LONG_INT", MPI_FLOAT_INT: "MPI_FLOAT_INT",
              MPI_DOUBLE_INT: "MPI_DOUBLE_INT", MPI_LONG_INT: "MPI_LONG_INT", MPI_SHORT_INT: "MPI_SHORT_INT",
              MPI_2INT: "MPI_2INT", MPI_LONG_DOUBLE_INT: "MPI_LONG_DOUBLE_INT", MPI_COMPLEX: "MPI_COMPLEX",
              MPI_DOUBLE_COMPLEX: "MPI_DOUBLE_COMPLEX", MPI_LOGICAL: "MPI_LOGICAL", MPI_REAL: "MPI_REAL",
              MPI_DOUBLE_PRECISION: "MPI_DOUBLE_PRECISION", MPI_INTEGER: "MPI_INTEGER",
              MPI_2INTEGER: "MPI_2INTEGER", MPI_2COMPLEX: "MPI_2COMPLEX", MPI_2DOUBLE_COMPLEX: "MPI_2DOUBLE_COMPLEX",
              MPI_2REAL: "MPI_2REAL", MPI_2DOUBLE_PRECISION: "MPI_2DOUBLE_PRECISION",
              MVX_FLOAT16: "MVX_FLOAT16", MVX_BFLOAT16: "MVX_BFLOAT16",
              MVX_FLOAT8_E4M3: "MVX_FLOAT8_E4M3", MVX_FLOAT8_E5M2: "MVX_FLOAT8_E5M2"}

# (op, type) pairs the reference defines (global_ops.c)
_INTS = [MPI_CHAR, MPI_UNSIGNED_CHAR, MPI_SHORT, MPI_UNSIGNED_SHORT, MPI_INT, MPI_UNSIGNED, MPI_LONG,
         MPI_UNSIGNED_LONG, MPI_LONG_LONG_INT, MPI_INTEGER]
_FLTS = [MPI_FLOAT, MPI_DOUBLE, MPI_LONG_DOUBLE, MPI_REAL, MPI_DOUBLE_PRECISION]
_PAIRS = [MPI_FLOAT_INT, MPI_DOUBLE_INT, MPI_LONG_INT, MPI_SHORT_INT, MPI_2INT, MPI_LONG_DOUBLE_INT,
          MPI_2INTEGER, MPI_2REAL, MPI_2DOUBLE_PRECISION]
DEFINED = {
    MPI_MAX: _INTS + _FLTS, MPI_MIN: _INTS + _FLTS,
    MPI_SUM: _INTS + _FLTS + [MPI_COMPLEX, MPI_DOUBLE_COMPLEX],
    MPI_PROD: _INTS + _FLTS + [MPI_COMPLEX, MPI_DOUBLE_COMPLEX],
    MPI_LAND: _INTS + _FLTS + [MPI_LOGICAL], MPI_LOR: _INTS + _FLTS + [MPI_LOGICAL],
    MPI_LXOR: _INTS + _FLTS + [MPI_LOGICAL],
    MPI_BAND: _INTS + [MPI_BYTE, MPI_LOGICAL], MPI_BOR: _INTS + [MPI_BYTE, MPI_LOGICAL],
    MPI_BXOR: _INTS + [MPI_BYTE, MPI_LOGICAL],
    MPI_MAXLOC: _PAIRS, MPI_MINLOC: _PAIRS,
}
# the extension types: the seven ops of MPI_FLOAT (DEFINED stays the reference's table)
_HALFS = [MVX_FLOAT16, MVX_BFLOAT16]
DEFINED_EXT = {op: list(_HALFS) for op in (MPI_MAX, MPI_MIN, MPI_SUM, MPI_PROD, MPI_LAND, MPI_LOR, MPI_LXOR)}
# the 8-bit floats, in a table of their own (DEFINED_EXT stays the 16-bit one)
_FP8S = [MVX_FLOAT8_E4M3, MVX_FLOAT8_E5M2]
DEFINED_EXT8 = {op: list(_FP8S) for op in DEFINED_EXT}
# the two f32-accumulating ops: the four narrow floats and nothing else
DEFINED_ACC32 = {op: _HALFS + _FP8S for op in (MVX_SUM_ACC32, MVX_PROD_ACC32)}
DEVICE_TYPES = sorted(NP_DTYPE)

# mvx_comm_set_call_kinds (include/mvx_embed.h)
KINDS_UNKNOWN = 0
KINDS_DEVICE = 1
KINDS_HOST = 2
