"""
ref_utils: the reference's small utilities, restated once.  Each test pins, for every tool that had a copy of its own, what that
copy returned on the inputs where the copies could have differed -- the values below are what the tools' copies gave before
they were merged -- and that the tools still reach the helper under the names they used.
"""

import json
import os

import numpy as np
import pytest
from PIL import Image

from megadetector_amd import change_detection as CD
from megadetector_amd import compare_batch_results as C
from megadetector_amd import postprocess_batch_results as PB
from megadetector_amd import ref_utils as RU
from megadetector_amd import repeat_detections as RD
from megadetector_amd import resize_coco_dataset as RC
from megadetector_amd import resize_images as R
from megadetector_amd import run_detector_batch as RDB
from megadetector_amd import run_tiled_inference as RTI
from megadetector_amd import separate_detections as SD
from megadetector_amd import visualize_db as VD
from megadetector_amd import visualize_video_output as VVO

LONG = 'x' * 300 + '.jpg'
#: name -> (with the defaults, replace_whitespace='_', force_lower=True)
CLEANED = {
    'sub\\deer one .jpg': ('subdeer one .jpg', 'subdeer_one_.jpg', 'subdeer one .jpg'),               # backslashes
    ' a / b c\t.JPG ': ('ab c.JPG', 'ab_c.JPG', 'ab c.jpg'),                                           # components are stripped
    'R\u00e9d  fox: 1/2': ('Red  fox 12', 'Red_fox_12', 'red  fox 12'),                                # NFKD; a run of blanks is one '_'
    'A\\B/C .Jpg': ('ABC .Jpg', 'ABC_.Jpg', 'abc .jpg'),                                               # both separators
    LONG: ('x' * 255, 'x' * 255, 'x' * 255),                                                           # cut to 255
}


def test_clean_filename_for_each_of_its_callers():
    assert PB.clean_filename is VVO.clean_filename is RTI.clean_filename is VD.clean_filename is RU.clean_filename
    for name, (plain, underscored, lowered) in CLEANED.items():
        assert RU.clean_filename(name) == plain                                                        # all three copies
        assert RU.clean_filename(name, replace_whitespace='_') == underscored                          # postprocess_batch_results' pages
        assert RU.clean_filename(name, force_lower=True) == lowered                                    # visualize_video_output, tiled folders
    # run_tiled_inference's tile names: not cut
    assert RU.clean_filename(LONG, char_limit=None, force_lower=True) == LONG and RU.clean_filename(LONG, char_limit=None) == LONG
    assert RU.clean_filename('Sub\\Deer.JPG', char_limit=None, force_lower=True) == 'subdeer.jpg'
    # visualize_db's category pages: lowered, then whitespace replaced
    assert [VD.category_page_name(n) for n in ('Bird "small"', 'Red  Fox', ' A\tb ')] == ['bird_small.html', 'red_fox.html', 'ab.html']
    # flatten_path keeps the separators until they become '~'
    assert PB.flatten_path is C.flatten_path is RU.flatten_path
    assert [RU.flatten_path(n) for n in list(CLEANED)[:4]] == ['sub~deer one .jpg', 'a~b c.JPG', 'Red  fox~ 1~2', 'A~B~C .Jpg']


def test_insert_before_extension_with_and_without_the_reference_assertions():
    assert PB.insert_before_extension is VVO.insert_before_extension is RU.insert_before_extension
    for name, dotted, underscored in (('a/b.mp4', 'a/b.x.mp4', 'a/b_x.mp4'), ('noext', 'noext.x', 'noext_x'),            # an empty extension
                                      ('.hidden', '.hidden.x', '.hidden_x'), ('a.b/c', 'a.b/c.x', 'a.b/c_x')):
        assert RU.insert_before_extension(name, 'x') == RU.insert_before_extension(name, 'x', check=True) == dotted
        assert RU.insert_before_extension(name, 'x', separator='_') == underscored
    assert RU.insert_before_extension('', 'x') == '.x'                                                 # postprocess_batch_results: unchecked
    with pytest.raises(AssertionError):                                                                # visualize_video_output: checked
        RU.insert_before_extension('', 'x', check=True)


def test_path_is_abs_with_and_without_the_leading_backslash():
    assert VVO.path_is_abs is SD.path_is_abs is RU.path_is_abs
    for p, video, separate in (('/a', True, True), ('C:\\x', True, True), ('a:', True, True), ('\\\\server\\x', True, False), ('\\x', True, False),
                               ('a', False, False), ('', False, False), ('ab', False, False), ('/', False, False)):
        assert RU.path_is_abs(p) is video, p                                                           # visualize_video_output
        assert RU.path_is_abs(p, leading_backslash=False) is separate, p                               # separate_detections


def test_find_images_absolute_and_relative(tmp_path):
    for name in ('b.JPG', 'a.png', 'notes.txt', 'no_dot', 'sub/c.webp', 'sub/deep/d.jpeg', 'sub/e.mp4'):
        os.makedirs(os.path.dirname(str(tmp_path / name)), exist_ok=True)
        open(str(tmp_path / name), 'wb').close()
    folder = str(tmp_path)
    assert CD.find_images is RU.find_images
    assert R.find_images(folder, recursive=True) == RU.find_images(folder, recursive=True, return_relative_paths=True)   # (its own, relative)
    # resize_images: relative, either depth
    assert RU.find_images(folder, recursive=True, return_relative_paths=True) == ['a.png', 'b.JPG', 'sub/c.webp', 'sub/deep/d.jpeg']
    assert RU.find_images(folder, return_relative_paths=True) == ['a.png', 'b.JPG']
    # change_detection and gray_scale: recursive, absolute
    assert RU.find_images(folder, recursive=True) == [folder + '/' + n for n in ('a.png', 'b.JPG', 'sub/c.webp', 'sub/deep/d.jpeg')]
    with pytest.raises(AssertionError, match='is not a folder'):
        RU.find_images(folder + '.none')
    # run_detector_batch keeps its own: a walk, four extensions, absolute, no assertion
    assert RDB.find_images(folder, recursive=True) == [folder + '/' + n for n in ('a.png', 'b.JPG', 'sub/deep/d.jpeg')]
    assert RU.IMG_EXTENSIONS == ('.jpg', '.jpeg', '.gif', '.png', '.tif', '.tiff', '.bmp', '.webp', '.avif') and RD.IMG_EXTENSIONS is RU.IMG_EXTENSIONS


def test_write_json_with_and_without_force_str(tmp_path):
    content = {'a': [1, 2.5, None], 'n\u00e9': 'x'}
    text = '{\n "a": [\n  1,\n  2.5,\n  null\n ],\n "n\\u00e9": "x"\n}'
    for k, write in enumerate((RU.write_json, RC.write_json, RDB.write_json, lambda p, c: RD.write_json(p, c, force_str=True))):
        path = str(tmp_path / 'made' / str(k) / 'out.json')                                            # (the folder is made)
        write(path, content)
        with open(path, newline='') as f:
            assert f.read() == text
    unserialisable = {'when': np.float32(1.5), 'where': tmp_path}
    RDB.write_json(str(tmp_path / 's.json'), unserialisable)                                           # run_detector_batch, the RDE files: str()
    assert json.load(open(str(tmp_path / 's.json'))) == {'when': '1.5', 'where': str(tmp_path)}
    RDB.write_json(str(tmp_path / 'i.json'), {'a': [1]}, indent=None)
    assert open(str(tmp_path / 'i.json')).read() == '{"a": [1]}'
    with pytest.raises(TypeError):                                                                     # resize_coco_dataset: json's own error
        RC.write_json(str(tmp_path / 't.json'), unserialisable)


def _exif_image(path, orientation=None, mode='RGB', **how):
    rng = np.random.default_rng(7)
    image = Image.fromarray(rng.integers(0, 255, (8, 12, 3), dtype=np.uint8)).convert(mode)
    exif = Image.Exif()
    exif[271] = 'a camera'
    if orientation is not None:
        exif[274] = orientation
    image.save(path, exif=exif, **how)
    return path


def test_open_image_is_lazy_and_turns_and_converts(tmp_path):
    assert PB.open_image is C.open_image is RC.open_image is VD.open_image is RU.open_image
    plain = RU.open_image(_exif_image(str(tmp_path / 'plain.jpg')))
    assert plain.format == 'JPEG' and plain.size == (12, 8)                                            # the opened image itself
    turned = RU.open_image(_exif_image(str(tmp_path / 'turned.jpg'), orientation=6))
    assert turned.format is None and turned.size == (8, 12)
    assert RU.open_image(_exif_image(str(tmp_path / 'mirrored.jpg'), orientation=2)).size == (12, 8)  # the assertion is swallowed, as there
    grey = RU.open_image(_exif_image(str(tmp_path / 'grey.jpg'), mode='L'))
    assert grey.mode == 'RGB' and grey.format is None
    Image.new('P', (4, 4)).save(str(tmp_path / 'palette.png'))
    with pytest.raises(AttributeError, match='uses unsupported mode P'):
        RU.open_image(str(tmp_path / 'palette.png'))
    with open(str(tmp_path / 'plain.jpg'), 'rb') as f:
        data = f.read()
    with open(str(tmp_path / 'cut.jpg'), 'wb') as f:
        f.write(data[:-12])                                                                            # (the end of the scan is missing)
    cut = RU.open_image(str(tmp_path / 'cut.jpg'))                                                     # lazy: a truncated file opens ...
    assert cut.size == (12, 8)
    with pytest.raises(OSError):                                                                       # ... and raises where it is loaded
        cut.load()


def test_exif_preserving_save_with_and_without_excluded_tags(tmp_path):
    assert SD.exif_preserving_save is R.exif_preserving_save is RC.exif_preserving_save is RU.exif_preserving_save
    source = _exif_image(str(tmp_path / 'source.jpg'), orientation=6, quality=50)
    tables = Image.open(source).quantization
    # separate_detections and resize_images: the block as it is; a JPEG keeps its tables, anything else is saved at 85
    RU.exif_preserving_save(Image.open(source), str(tmp_path / 'kept.jpg'))
    kept = Image.open(str(tmp_path / 'kept.jpg'))
    assert kept.quantization == tables and dict(kept.getexif()) == {271: 'a camera', 274: 6}
    resized = Image.open(source).resize((6, 4))
    RU.exif_preserving_save(resized, str(tmp_path / 'resized.jpg'))
    RU.exif_preserving_save(Image.open(source).resize((6, 4)), str(tmp_path / 'resized_95.jpg'), quality=95)
    resized.save(str(tmp_path / 'at_85.jpg'), quality=85, exif=resized.getexif())
    assert open(str(tmp_path / 'resized.jpg'), 'rb').read() == open(str(tmp_path / 'at_85.jpg'), 'rb').read()
    assert Image.open(str(tmp_path / 'resized_95.jpg')).quantization != Image.open(str(tmp_path / 'resized.jpg')).quantization
    # resize_coco_dataset: without the tags it names
    RU.exif_preserving_save(Image.open(source).resize((6, 4)), str(tmp_path / 'without.jpg'), tags_to_exclude=(RU.ORIENTATION,))
    assert dict(Image.open(str(tmp_path / 'without.jpg')).getexif()) == {271: 'a camera'}
    assert dict(RU.exif_without(Image.open(source), (271, 274, 999))) == {}
    # what the first save refuses is saved once more without the quality: a PNG has none to 'keep'
    RU.exif_preserving_save(Image.open(source), str(tmp_path / 'copy.png'))
    assert Image.open(str(tmp_path / 'copy.png')).size == (12, 8)


def test_quality_argument():
    assert R.quality_argument is VVO.quality_argument is RU.quality_argument
    assert RU.quality_argument('keep') == 'keep' and RU.quality_argument('75') == 75
    with pytest.raises(ValueError):
        RU.quality_argument('best')
