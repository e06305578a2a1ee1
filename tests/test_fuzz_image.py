"""The image reader of `(texture ...)` blocks (csrc/host/image_reader.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer:
`make -C pearray_amd/csrc san` builds it into the stand-alone driver (san/san_driver.cpp, `prc_san --image`), and tools/fuzz_image.py
feeds that driver truncations and byte mutations of PNG and PFM seeds it encodes itself, with a fixed seed.  A finding aborts the
driver; a clean run answers every input with 0 or one of the reader's error codes."""
import image_files as imf


def test_seed_images_load_and_mutants_never_trip_a_sanitizer():
    finding, rep = imf.fuzz_image.run(n=400, seed=7)
    assert not finding, rep
    assert rep["seed_codes"] == ["0"] and rep["seeds"] == 12, rep      # every unmutated seed (each colour type and depth, three PFMs) loads
    assert rep["answered"] == rep["inputs"] == 412
    assert set(rep["status_codes"]) <= {"0", "-1", "-4", "-5"}, rep   # loaded, invalid, unsupported, i/o -- never anything else
    # the mutants reach the success path and each kind of refusal
    assert rep["status_codes"].get("0", 0) >= 10 and rep["status_codes"].get("-1", 0) >= 100 and rep["status_codes"].get("-5", 0) >= 20, rep
