function pathLoss = configFreeSpaceModel(carrierFreq, bsPosition, uePosition)
%CONFIGFREESPACEMODEL  Drop-in replacement body for +communication/+pathlossModels/configFreeSpaceModel.m: 20*log10(4*pi*R/lambda) [dB],
%   negative values clamped to 0 as fspl does.
    pathLoss = isac_mex('pathLoss', 'fspl', double(carrierFreq), [], double(bsPosition(:)).', double(uePosition(:)).');
end
