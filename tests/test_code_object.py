"""CPU: the reader of the library's gfx950 code object (tests/code_object.py) — its notes parser on a text written out here, and on the built
library against the notes themselves, against the disassembly and, where PyYAML is installed, against a YAML parse of the same document."""
import re

import pytest

import code_object

KEYS_IN_USE = (".agpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size", ".sgpr_count", ".sgpr_spill_count", ".vgpr_count",
               ".vgpr_spill_count", ".wavefront_size")

# two entries as llvm-readelf --notes prints them: keys sorted, so .agpr_count and .group_segment_fixed_size stand BEFORE .name
NOTES = """\
Displaying notes found in: .note
  Owner                Data size \tDescription
  AMDGPU               0x00000400\tNT_AMDGPU_METADATA (AMDGPU Metadata)
    AMDGPU Metadata:
        ---
amdhsa.kernels:
  - .agpr_count:     4
    .args:
      - .actual_access:  read_only
        .address_space:  global
        .name:           not_a_kernel
        .offset:         0
        .size:           8
        .value_kind:     global_buffer
      - .offset:         8
        .size:           4
        .value_kind:     by_value
    .group_segment_fixed_size: 0
    .kernarg_segment_align: 8
    .kernarg_segment_size: 12
    .language:       OpenCL C
    .language_version:
      - 2
      - 0
    .max_flat_workgroup_size: 256
    .name:           _ZN3lfi5firstEPKhi
    .private_segment_fixed_size: 0
    .sgpr_count:     16
    .sgpr_spill_count: 0
    .symbol:         _ZN3lfi5firstEPKhi.kd
    .uniform_work_group_size: 1
    .uses_dynamic_stack: false
    .vgpr_count:     44
    .vgpr_spill_count: 0
    .wavefront_size: 64
  - .agpr_count:     16
    .args:
      - .offset:         0
        .size:           136
        .value_kind:     by_value
    .group_segment_fixed_size: 12960
    .kernarg_segment_align: 8
    .kernarg_segment_size: 136
    .language:       OpenCL C
    .language_version:
      - 2
      - 0
    .max_flat_workgroup_size: 256
    .name:           _ZN3lfi6secondILi0ELb1EEEvNS_4ArgsE
    .private_segment_fixed_size: 24
    .sgpr_count:     43
    .sgpr_spill_count: 0
    .symbol:         _ZN3lfi6secondILi0ELb1EEEvNS_4ArgsE.kd
    .uniform_work_group_size: 1
    .uses_dynamic_stack: false
    .vgpr_count:     62
    .vgpr_spill_count: 3
    .wavefront_size: 64
amdhsa.target:   amdgcn-amd-amdhsa--gfx950
amdhsa.version:
  - 1
  - 2
...
"""


def _name_first_parser(notes, keys):
    """The loop eleven tests used to carry: a record begins at its .name line, so the keys that sort before .name are filed under the kernel
    before (the first kernel's are dropped)"""
    kernels, name = {}, None
    for line in notes.splitlines():
        line = line.strip()
        if line.startswith(".name:"):
            name = line.split(":", 1)[1].strip()
            kernels[name] = {}
        elif name and ":" in line and line.split(":")[0] in keys:
            kernels[name][line.split(":")[0]] = int(line.split(":")[1])
    return kernels


def test_every_field_lands_under_its_own_name():
    """The counter-example: the name-first loop hands the SECOND kernel's 12960 bytes of LDS to the first (whose own 0 it files under an
    argument's .name, taken for a kernel) and leaves the second without any; .agpr_count, behind the list item's dash, it never sees.
    The reader files every scalar field of an entry under that entry's .name, skips the entries of .args and the items of
    .language_version, and stops at amdhsa.target."""
    first, second = "_ZN3lfi5firstEPKhi", "_ZN3lfi6secondILi0ELb1EEEvNS_4ArgsE"
    got = code_object.parse_notes(NOTES)
    assert list(got) == [first, second]
    assert got[first] == {
        ".agpr_count": 4, ".group_segment_fixed_size": 0, ".kernarg_segment_align": 8, ".kernarg_segment_size": 12, ".language": "OpenCL C",
        ".max_flat_workgroup_size": 256, ".name": first, ".private_segment_fixed_size": 0, ".sgpr_count": 16, ".sgpr_spill_count": 0,
        ".symbol": first + ".kd", ".uniform_work_group_size": 1, ".uses_dynamic_stack": False, ".vgpr_count": 44, ".vgpr_spill_count": 0,
        ".wavefront_size": 64}
    assert got[second] == {
        ".agpr_count": 16, ".group_segment_fixed_size": 12960, ".kernarg_segment_align": 8, ".kernarg_segment_size": 136,
        ".language": "OpenCL C", ".max_flat_workgroup_size": 256, ".name": second, ".private_segment_fixed_size": 24, ".sgpr_count": 43,
        ".sgpr_spill_count": 0, ".symbol": second + ".kd", ".uniform_work_group_size": 1, ".uses_dynamic_stack": False, ".vgpr_count": 62,
        ".vgpr_spill_count": 3, ".wavefront_size": 64}
    old = _name_first_parser(NOTES, KEYS_IN_USE)
    assert "not_a_kernel" in old
    assert old[first][".group_segment_fixed_size"] == 12960 and ".group_segment_fixed_size" not in old[second]   # the second kernel's
    assert old["not_a_kernel"][".group_segment_fixed_size"] == 0                                                  # the first kernel's
    assert ".agpr_count" not in old[first] and ".agpr_count" not in old[second]   # "- .agpr_count" opens the entry: never recognised
    assert old[first][".vgpr_count"] == 44 and old[second][".vgpr_count"] == 62                  # the keys behind .name it got right


def test_named_is_exact():
    records = {"_ZN3lfi11yuvs_expandILi0ELb0EEEvNS_10YuvsInArgsE": 1, "_ZN3lfi19yuvs_derived_expandILi0ELb0EEEvNS_15YuvsDerivedArgsE": 2,
               "_ZN3lfi16yuvs_expand_moreILi0EEEvi": 3, "_ZN3lfi11yuvs_expandEPKhi": 4, "_ZN5other11yuvs_expandEPKhi": 5,
               "_ZN3lfi11yuvs_expandILi0ELb0EEEvNS_10YuvsInArgsE.kd": 6, "_ZN3lfi11yuvs_expandXEPKhi": 7}
    assert sorted(code_object.named(records, "yuvs_expand").values()) == [1, 4, 6]
    assert list(code_object.named(records, "yuvs_derived_expand").values()) == [2]
    assert code_object.named(records, "expand") == {}


needs_tools = pytest.mark.skipif(not code_object.have_tools(), reason="ROCm LLVM tools not installed")


@needs_tools
def test_one_record_per_kernel_descriptor(native):
    lib = native.build.HIP_LIB
    kernels = code_object.kernels(lib)
    descriptors = re.findall(r"^    \.symbol:\s+(\S+)\.kd$", code_object.notes(lib), re.M)
    assert len(descriptors) > 100 and sorted(descriptors) == sorted(kernels)
    for name, record in kernels.items():
        assert record[".name"] == name and record[".symbol"] == name + ".kd"
        assert all(type(record[key]) is int for key in KEYS_IN_USE), (name, record)
    # every kernel has code under its own symbol
    assert set(kernels) <= set(code_object.bodies(lib))


@needs_tools
def test_the_code_object_is_cut_out_once(native):
    lib = native.build.HIP_LIB
    assert code_object.path(lib) == code_object.path(lib) and code_object.kernels(lib) is code_object.kernels(lib)
    assert code_object.bodies(lib) is code_object.bodies(lib)
    assert open(code_object.path(lib), "rb").read(4) == b"\x7fELF"


@needs_tools
def test_yuvs_expand_is_not_yuvs_derived_expand(native):
    kernels = code_object.kernels(native.build.HIP_LIB)
    expand, derived = code_object.named(kernels, "yuvs_expand"), code_object.named(kernels, "yuvs_derived_expand")
    assert len(expand) == 4 and len(derived) == 4 and not set(expand) & set(derived)
    assert not any("yuvs_derived_expand" in k for k in expand)
    assert len(code_object.named(code_object.bodies(native.build.HIP_LIB), "yuvs_expand")) == 4
    # what the name-first loop swapped (yuv_surfaces.hpp's kernels hold no LDS, yuv_derived.hpp's stage their blocks there)
    assert all(v[".group_segment_fixed_size"] == 0 for v in expand.values())
    assert all(v[".group_segment_fixed_size"] > 0 for v in derived.values())


@needs_tools
def test_records_equal_a_yaml_parse_of_the_notes(native):
    yaml = pytest.importorskip("yaml")
    lib = native.build.HIP_LIB
    text = code_object.notes(lib)
    document = yaml.safe_load(text[text.index("amdhsa.kernels:"):text.rindex("\n...")])
    want = {entry[".name"]: {k: v for k, v in entry.items() if not isinstance(v, (list, dict))} for entry in document["amdhsa.kernels"]}
    assert len(want) == len(document["amdhsa.kernels"])
    assert code_object.kernels(lib) == want
