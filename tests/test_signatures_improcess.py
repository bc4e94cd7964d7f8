"""improcess mirrors every computation of the reference's improcess namespace: each name recorded in
tests/golden/reference_signatures.json["improcess"] exists with the reference's parameter names, order and defaults.
Only detect_long_lines (Canny + randomised probabilistic Hough + plt.show()) stays out."""
import json

from tests.test_signatures import SIGNATURES, _params

OUT_OF_SCOPE = {"detect_long_lines"}


def test_improcess_signatures_complete():
    with open(SIGNATURES) as f:
        ref = json.load(f)["improcess"]
    from das4whales_amd import improcess
    assert OUT_OF_SCOPE <= set(ref)
    for name in OUT_OF_SCOPE:
        assert not hasattr(improcess, name), "%s is out of scope: no stub" % name
    checked = 0
    for name, params in sorted(ref.items()):
        if name in OUT_OF_SCOPE:
            continue
        assert hasattr(improcess, name), "improcess.%s is missing" % name
        assert _params(getattr(improcess, name)) == [tuple(p) for p in params], name
        checked += 1
    assert checked == len(ref) - 1 >= 12
