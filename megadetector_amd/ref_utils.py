"""
The reference's small utilities (utils/path_utils.py, utils/ct_utils.py, visualization/visualization_utils.py), restated once
for every tool that needs them.  Where the tools' earlier copies differed, the difference is an argument here, and each
caller passes what its copy did.  run_detector_batch.find_images is not here: it walks the folder, knows four extensions,
returns absolute paths and asserts nothing -- another function.
"""

import glob
import json
import os
import re
import unicodedata

VALID_FILENAME_CHARS = '~-_.() abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789'      # utils/path_utils.py:46
SEPARATOR_CHARS = ':\\/'
CHAR_LIMIT = 255
#: reference path_utils.IMG_EXTENSIONS
IMG_EXTENSIONS = ('.jpg', '.jpeg', '.gif', '.png', '.tif', '.tiff', '.bmp', '.webp', '.avif')
ORIENTATION = 274               # the id of 'Orientation' in PIL.ExifTags
DEFAULT_SAVE_QUALITY = 85       # visualization_utils.py:199 exif_preserving_save(..., default_quality=85)


# ---- utils/path_utils.py -----------------------------------------------------------------------------------------------------------

def clean_filename(filename, allow_list=VALID_FILENAME_CHARS, char_limit=CHAR_LIMIT, force_lower=False, replace_whitespace=None):
    """path_utils.clean_filename :568 (with remove_trailing_leading_whitespace, its default): every path component stripped,
    ASCII characters of allow_list only, cut to char_limit (None: not cut), then lowered, then whitespace replaced"""
    separator = '\\' if '\\' in filename else '/'
    filename = separator.join([c.strip() for c in filename.replace('\\', '/').split('/')])
    cleaned = unicodedata.normalize('NFKD', filename).encode('ASCII', 'ignore').decode()
    cleaned = ''.join([c for c in cleaned if c in allow_list])
    if char_limit is not None:
        cleaned = cleaned[:char_limit]
    if force_lower:
        cleaned = cleaned.lower()
    if replace_whitespace is not None:
        cleaned = re.sub(r'\s+', replace_whitespace, cleaned)
    return cleaned


def flatten_path(pathname):
    """path_utils.flatten_path: clean_path, then every separator becomes '~'"""
    s = clean_filename(pathname, allow_list=VALID_FILENAME_CHARS + SEPARATOR_CHARS)
    for c in SEPARATOR_CHARS:
        s = s.replace(c, '~')
    return s


def insert_before_extension(filename, s, separator='.', check=False):
    """path_utils.insert_before_extension :254 for a string `s` that is not empty.  check: the reference's two assertions,
    which visualize_video_output makes and postprocess_batch_results' page names never needed"""
    name, ext = os.path.splitext(filename)
    output_string = '{}{}{}{}'.format(name, separator, s, ext)
    if check:
        assert len(filename) > 0
        assert output_string != filename, 'Input and output filenames are identical'
    return output_string


def path_is_abs(p, leading_backslash=True):
    """path_utils.path_is_abs :334.  leading_backslash=False: without its case of a path that starts with a backslash, as
    separate_detections has always checked its results files"""
    return (len(p) > 1) and (p[0] == '/' or p[1] == ':' or (leading_backslash and p[0] == '\\'))


def find_images(dirname, recursive=False, return_relative_paths=False):
    """path_utils.find_images(dirname, recursive, return_relative_paths, convert_slashes=True): a glob of *.*, the
    reference's extension list, sorted, forward slashes"""
    assert os.path.isdir(dirname), '{} is not a folder'.format(dirname)
    if recursive:
        strings = glob.glob(os.path.join(dirname, '**', '*.*'), recursive=True)
    else:
        strings = glob.glob(os.path.join(dirname, '*.*'))
    image_files = [s for s in strings if os.path.splitext(s)[1].lower() in IMG_EXTENSIONS]
    if return_relative_paths:
        image_files = [os.path.relpath(fn, dirname) for fn in image_files]
    return [fn.replace('\\', '/') for fn in sorted(image_files)]


# ---- utils/ct_utils.py -------------------------------------------------------------------------------------------------------------

def write_json(path, content, indent=1, force_str=False):
    """ct_utils.write_json :210-251.  force_str: what json does not serialise is written as its str()"""
    parent_dir = os.path.dirname(path)
    if len(parent_dir) > 0:
        os.makedirs(parent_dir, exist_ok=True)
    with open(path, 'w', newline='\n', encoding='utf-8') as f:
        json.dump(content, f, indent=indent, default=str if force_str else None, ensure_ascii=True)


# ---- visualization/visualization_utils.py ------------------------------------------------------------------------------------------

def open_image(input_file):
    """visualization_utils.open_image :103-176 for a local file: feed.load_image without the load -- the mode check, 'RGBA' /
    'L' converted, the EXIF rotation; lazy, as there (no pixel is decoded unless one of the two made a new image, and a
    truncated file raises where it is resized)"""
    from PIL import Image
    from .feed import EXIF_IMAGE_ROTATIONS
    image = Image.open(input_file)
    if image.mode not in ('RGBA', 'RGB', 'L', 'I;16'):
        raise AttributeError('Image {} uses unsupported mode {}'.format(input_file, image.mode))
    if image.mode in ('RGBA', 'L'):
        image = image.convert(mode='RGB')
    try:
        exif = image._getexif()
        orientation = exif.get(ORIENTATION, None)
        if (orientation is not None) and (orientation != 1):
            assert orientation in EXIF_IMAGE_ROTATIONS, 'Mirrored rotations are not supported'
            image = image.rotate(EXIF_IMAGE_ROTATIONS[orientation], expand=True)
    except Exception:
        pass
    return image


def exif_without(pil_image, tag_ids):
    """_remove_exif_tags: the image's getexif() with the tags popped"""
    exif = pil_image.getexif()
    if exif is not None:
        for tag in tag_ids:
            exif.pop(tag, None)
    return exif


def exif_preserving_save(pil_image, output_file, quality='keep', default_quality=DEFAULT_SAVE_QUALITY, tags_to_exclude=None):
    """visualization_utils.exif_preserving_save :196-301: the EXIF block kept, without tags_to_exclude (a tuple of tag ids
    here); the quality 'kept' only for a JPEG source; once more without the quality, then without the EXIF block"""
    exif = pil_image.getexif()
    if (exif is not None) and (tags_to_exclude is not None):
        exif = exif_without(pil_image, tags_to_exclude)
    if pil_image.format != 'JPEG':
        if quality == 'keep':
            quality = default_quality
    for kwargs in ({'quality': quality}, {}):
        try:
            if exif is not None:
                pil_image.save(output_file, exif=exif, **kwargs)
            else:
                pil_image.save(output_file, **kwargs)
            return
        except Exception:
            pass
    pil_image.save(output_file)


def quality_argument(s):
    """argparse's type of a --quality option: 'keep', or an integer JPEG quality"""
    return s if s == 'keep' else int(s)
